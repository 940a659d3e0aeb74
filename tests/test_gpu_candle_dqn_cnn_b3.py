"""set_arithmetic("bf16x3_6") of the candle DQN's AtariCnn form: conv2 / conv3 forward on the bf16 matrix cores in the update and on the
layer acting path (k_fwd_c23_b3 from per-set weight planes) and on BDR_ACT_PATH_IMAGE (k_cnn_act_trunk_b3).

Every layer is checked on the device's own input of that layer (probes a1, a2, a3) against the float64 reference of
tests/dqn_forward_reference.py with split=True: its per-element bound, SPLIT_C * S for the three dropped products, and its LAMBDA -
this file has no tolerance of its own.  Both kernels sum k ascending in steps of 16 with the six kept products smallest first, the
order restatement(..., split=True) evaluates, so LAMBDA stands as it is.  All of it fails on a library without the entry point."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import candle_dqn_cnn_restatement as R  # noqa: E402
import candle_dqn_restatement as RM  # noqa: E402
import dqn_forward_reference as F  # noqa: E402

pytestmark = pytest.mark.gpu
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
UPDATES = ((1, 4, 6, False), (3, 1, 18, True), (33, 4, 2, False))   # (B, n_stack, A, double_dqn): one image, three instances, a ragged batch
PROBES = ("pred", "q_next", "tgt")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


@functools.lru_cache(maxsize=None)
def case(Bn, ns, A, double):
    spec = R.CandleDqnCnnSpec(ns, A, adamw=ADAMW, double_dqn=double)
    return spec, spec.init_params(10 * Bn + ns), R.make_batch(spec, Bn, 3 * Bn + A)


def agent(B, spec, params, bsz, arithmetic="bf16x3_6", path="layers"):
    a = B.CandleDqn.build(spec.to_config(B, bsz, device=0))
    a.set_arithmetic(arithmetic)
    a.set_params(params[0], "qnet"); a.set_params(params[1], "qnet_tgt")
    a.set_act_path(path)
    return a


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def check_layers(spec, qnet, obs, layers, with_a1=False):
    """a2 from the probed a1 and a3 from the probed a2 (and a1 from the frames) under the reference's bound, element by element"""
    n = len(obs)
    inp = dict(params=F.unflat(qnet, R.var_shapes(spec.n_stack, spec.n_actions)), obs=obs.reshape(n, spec.n_stack, 84, 84), a1=layers["a1"], a2=layers["a2"])
    names = (("a1",) if with_a1 else ()) + tuple(k for k in ("a2", "a3") if k in layers)
    v = F.check_all(F.reference(inp, split=True, only=names), {k: layers[k] for k in names}, F.LAMBDA)
    print({k: round(x.sharp_ratio, 3) for k, x in v.items()})


def probed(a, n, names=("a1", "a2", "a3")):
    return {k: a.probe(k, n) for k in names}


@pytest.mark.parametrize("Bn,ns,A,double", UPDATES)
def test_update_forward_layer_by_layer(B, Bn, ns, A, double):
    spec, params, batch = case(Bn, ns, A, double)
    a, twin = agent(B, spec, params, Bn), agent(B, spec, params, Bn, "f32_exact")
    a.update_on_batch(*batch); twin.update_on_batch(*batch)
    got = probed(a, Bn)
    assert (bits(got["a1"]) == bits(twin.probe("a1", Bn))).all()             # conv1 is the exact agent's kernel
    assert not (bits(got["a2"]) == bits(twin.probe("a2", Bn))).all()         # conv2 is not
    check_layers(spec, params[0], batch[0], got)
    a.close(); twin.close()


@pytest.mark.parametrize("ns,A", ((1, 2), (4, 6)))
@pytest.mark.parametrize("n", (1, 3, 32))
def test_image_trunk_layer_by_layer(B, ns, A, n):
    spec, params, _ = case(3, ns, A, False)
    obs = R.make_batch(spec, n, 7 * n + A)[0]
    a = agent(B, spec, params, n, path="image")
    a.keep_layers(True)
    a.qvalues(obs)
    check_layers(spec, params[0], obs, probed(a, n), with_a1=True)
    a.keep_layers(False)
    a.qvalues(obs)
    with pytest.raises(B.BdrError, match="keep_layers"):
        a.probe("a1", n)
    a.close()


def test_33_rows_take_the_layer_launches_bit_for_bit(B):
    spec, params, _ = case(3, 4, 6, False)
    obs = R.make_batch(spec, 33, 5)[0]
    a, b = agent(B, spec, params, 33, path="image"), agent(B, spec, params, 33)
    assert (bits(a.qvalues(obs)) == bits(b.qvalues(obs))).all()
    a.close(); b.close()


def test_the_image_trunk_sums_as_the_layer_path_does(B):
    """the summation-order statement of cnn_act_img.hpp: from the SAME a1, k_cnn_act_trunk_b3 gives k_fwd_c23_b3's a2 and a3 to the
    bit.  The two conv1 kernels order their sums differently, so the case makes conv1 exact in any order: W1 in multiples of 1/64
    up to 8/64 and b1 = 0 - every partial sum of pixel x weight is an integer below 2^24 in units of 1/64 - with generic W2, W3."""
    spec, params, _ = case(3, 4, 6, False)
    sl = R.var_slices(4, 6)
    q = params[0].copy()
    q[sl["c1.weight"]] = np.random.default_rng(3).integers(-8, 9, sl["c1.weight"].stop - sl["c1.weight"].start) / 64.0
    q[sl["c1.bias"]] = 0.0
    obs = R.make_batch(spec, 32, 11)[0]
    a, b = agent(B, spec, (q, q), 32, path="image"), agent(B, spec, (q, q), 32)
    a.keep_layers(True)
    a.qvalues(obs); b.qvalues(obs)
    got, want = probed(a, 32), probed(b, 32)
    assert got["a1"].any()
    for k in ("a1", "a2", "a3"):
        assert (bits(got[k]) == bits(want[k])).all(), k
    a.close(); b.close()


def test_planes_follow_every_writer_of_the_conv_parameters(B):
    """two tracking updates (the optimizer launch re-splits what it steps, both sets), then set_params: after each, a2 of an acting call
    is held against the parameters as read back; the target set's planes, which no probe of instance 0 shows, against a twin that
    re-splits the same parameters from scratch - its next update must give the same pred, q_next and tgt to the bit"""
    Bn, ns, A, double = UPDATES[1]
    spec, params, batch = case(Bn, ns, A, double)
    a = agent(B, spec, params, Bn)

    def acting_a2():
        a.qvalues(batch[0])
        check_layers(spec, a.get_params("qnet"), batch[0], probed(a, Bn, ("a1", "a2")))
    for _ in range(2):
        a.update_on_batch(*batch)
        acting_a2()
    twin = agent(B, spec, (a.get_params("qnet"), a.get_params("qnet_tgt")), Bn)
    a.update_on_batch(*batch); twin.update_on_batch(*batch)
    for k in PROBES:
        assert (bits(a.probe(k, Bn)) == bits(twin.probe(k, Bn))).all(), k
    other = spec.init_params(77)
    a.set_params(other[0], "qnet"); a.set_params(other[1], "qnet_tgt")
    acting_a2()
    a.close(); twin.close()


def test_one_update_takes_fifteen_launches_plus_the_gather(B):
    spec, params, batch = case(3, 4, 6, False)
    a = agent(B, spec, params, 3)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=1), (spec.row_bytes,), np.uint8, (1,), np.int64)
    rb.push(batch[0], batch[1].reshape(-1, 1), *batch[2:])
    a.opt(rb)                                     # (the first forward splits both sets: two conv_planes launches, once)
    a.profile_enable(True)
    a.opt(rb)
    a.sync()
    names = [k for k, _ in a.profile_read()]
    a.profile_enable(False)
    assert names == ["sample", "fwd_conv", "fwd_conv", "fwd", "fwd", "cdqn_td", "dx", "dx", "dw", "reduce_adam",
                     "conv3_dw", "conv3_dx", "conv2_dw", "conv2_dx", "conv1_dw", "conv_reduce_adam"], names
    a.close(); rb.close()


def test_what_the_switch_and_the_group_rule_refuse(B):
    spec, params, _ = case(3, 4, 6, False)
    a, b, c = agent(B, spec, params, 3, "f32_exact"), agent(B, spec, params, 3), agent(B, spec, params, 3, "f32_exact")
    for value in (-1, 2):
        assert B._lib.lib().bdr_candle_dqn_cnn_set_arithmetic(a.handle, value) == 1 and b"unknown arithmetic" in B._lib.lib().bdr_last_error()
    b.set_arithmetic("bf16x3_6")                                   # the value it has: accepted
    with pytest.raises(B.BdrError, match="stays so"):              # one way
        b.set_arithmetic("f32_exact")
    with pytest.raises(B.BdrError, match="BDR_ARITH_BF16X3_6"):
        B.CandleDqnCnnGroup([a, b])
    with pytest.raises(B.BdrError, match="split-operand.*bdr_candle_dqn_cnn_set_arithmetic"):   # the constructor names the switch
        B.CandleDqn.build(spec.to_config(B, 3, device=0, arithmetic="bf16x3_6"))
    mlp = B.CandleDqn.build(RM.CandleDqnSpec(5, 4, (32,), adamw=ADAMW).to_config(B, 2, device=0))
    with pytest.raises(B.BdrError, match="AtariCnn"):
        mlp.set_arithmetic("bf16x3_6")
    mlp.close(); b.close()
    g = B.CandleDqnCnnGroup([a, c])
    with pytest.raises(B.BdrError, match="member of a group"):
        c.set_arithmetic("bf16x3_6")
    g.close()
