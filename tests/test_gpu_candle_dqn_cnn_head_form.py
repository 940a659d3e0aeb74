"""set_head_form("splitk") of the candle DQN's AtariCnn form: l1 + l2 of every instance and row tile in one launch, k_cdqn_head_fwd
(csrc/cdqn_head_fwd.hpp), in the update and on the layer acting path.

h1 is checked on the device's own a3 and q on the device's own h1 (probes a3, h1, q) against the float64 reference of
tests/dqn_forward_reference.py: its per-element bound and its LAMBDA - this file has no tolerance of its own.  The instances no probe
shows and the acting path are held bit for bit against twins.  All of it fails on a library without the entry point and probes 8 / 9."""
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
# (B, n_stack, A, double_dqn): one row; three instances and 18 actions; a ragged second row tile; three row tiles, the last ragged
UPDATES = ((1, 4, 6, False), (3, 1, 18, True), (33, 4, 2, False), (65, 4, 6, False))
NAMES = ["sample", "fwd_conv", "fwd_conv", "fwd_conv", "fwd_head", "cdqn_td", "dx", "dx", "dw", "reduce_adam",
         "conv3_dw", "conv3_dx", "conv2_dw", "conv2_dx", "conv1_dw", "conv_reduce_adam"]


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


def agent(B, spec, params, bsz, form="splitk", arithmetic="f32_exact"):
    a = B.CandleDqn.build(spec.to_config(B, bsz, device=0))
    a.set_arithmetic(arithmetic)
    a.set_head_form(form)
    a.set_params(params[0], "qnet"); a.set_params(params[1], "qnet_tgt")
    a.set_act_path("layers")
    return a


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("Bn,ns,A,double", UPDATES)
def test_update_head_layer_by_layer(B, Bn, ns, A, double):
    """largest |err| / (sqrt(n) u S) measured over the four cases: h1 0.007, q 0.029, against LAMBDA 1.0 and 1.0"""
    spec, params, batch = case(Bn, ns, A, double)
    a, twin = agent(B, spec, params, Bn), agent(B, spec, params, Bn, "layers")
    a.update_on_batch(*batch); twin.update_on_batch(*batch)
    got = {k: a.probe(k, Bn) for k in ("a3", "h1", "q")}
    inp = dict(params=F.unflat(params[0], R.var_shapes(ns, A)), a3=got["a3"], h1=got["h1"])
    v = F.check_all(F.reference(inp, only=("h1", "q")), {k: got[k] for k in ("h1", "q")}, F.LAMBDA)
    print({k: round(x.sharp_ratio, 3) for k, x in v.items()})
    assert got["h1"].any() and (bits(got["h1"]) != bits(twin.probe("h1", Bn))).any()   # seven slices, not one: the switch does something
    a.close(); twin.close()


@pytest.mark.parametrize("Bn,ns,A,double", (UPDATES[1], UPDATES[2]))
def test_every_instance_and_acting_equal_the_update(B, Bn, ns, A, double):
    spec, params, batch = case(Bn, ns, A, double)
    obs, act, nobs = batch[0], batch[1], batch[2]
    a, on, tg = agent(B, spec, params, Bn), agent(B, spec, params, Bn), agent(B, spec, (params[1], params[1]), Bn)
    a.update_on_batch(*batch)
    q_tg = tg.qvalues(nobs)
    y = np.argmax(on.qvalues(nobs) if double else q_tg, axis=1)            # the first maximum
    rows = np.arange(Bn)
    assert (a.probe("y", Bn) == y).all()
    assert (bits(a.probe("q_next", Bn)) == bits(q_tg[rows, y])).all()
    assert (bits(a.probe("pred", Bn)) == bits(on.qvalues(obs)[rows, act])).all()
    for x in (a, on, tg):
        x.close()


def test_the_counters_are_armed_again(B):
    spec, params, batch = case(*UPDATES[2])
    a = agent(B, spec, params, 33)
    a.update_on_batch(*batch); a.update_on_batch(*batch)
    q = a.qvalues(batch[0])
    fresh = agent(B, spec, (a.get_params("qnet"), a.get_params("qnet_tgt")), 33)
    assert (bits(q) == bits(fresh.qvalues(batch[0]))).all()
    a.update_on_batch(*batch); fresh.update_on_batch(*batch)
    for k in ("pred", "q_next", "tgt"):
        assert (bits(a.probe(k, 33)) == bits(fresh.probe(k, 33))).all(), k
    a.close(); fresh.close()


@pytest.mark.parametrize("arithmetic", ("f32_exact", "bf16x3_6"))
def test_one_fwd_head_where_the_two_fwd_stood(B, arithmetic):
    spec, params, batch = case(3, 4, 6, False)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=1), (spec.row_bytes,), np.uint8, (1,), np.int64)
    rb.push(batch[0], batch[1].reshape(-1, 1), *batch[2:])

    def names(a):
        a.opt(rb)                                 # (buffers of the form; the split arithmetic's planes)
        a.profile_enable(True)
        a.opt(rb)
        a.sync()
        got = [k for k, _ in a.profile_read()]
        a.profile_enable(False)
        return got
    a, back = agent(B, spec, params, 3, arithmetic=arithmetic), agent(B, spec, params, 3, arithmetic=arithmetic)
    want = [k for i, k in enumerate(NAMES) if not (arithmetic == "bf16x3_6" and i == 3)]   # conv2 + conv3 are one launch there
    assert names(a) == want, names(a)
    back.opt(rb)
    back.set_head_form("layers")                  # the way back: the layer form's list, as it always was
    k = want.index("fwd_head")
    assert names(back) == want[:k] + ["fwd", "fwd"] + want[k + 1:]
    a.close(); back.close(); rb.close()


def test_what_the_switch_the_group_rule_and_the_probes_refuse(B):
    spec, params, _ = case(3, 4, 6, False)
    a, b, c = agent(B, spec, params, 3, "layers"), agent(B, spec, params, 3), agent(B, spec, params, 3, "layers")
    for value in (-1, 2):
        assert B._lib.lib().bdr_candle_dqn_cnn_set_head_form(a.handle, value) == 1 and b"unknown head form" in B._lib.lib().bdr_last_error()
    with pytest.raises(B.BdrError, match="BDR_HEAD_FORM_SPLITK"):
        B.CandleDqnCnnGroup([a, b])
    mlp = B.CandleDqn.build(RM.CandleDqnSpec(5, 4, (32,), adamw=ADAMW).to_config(B, 2, device=0))
    with pytest.raises(B.BdrError, match="AtariCnn"):
        mlp.set_head_form("splitk")
    mlp.close()
    obs = R.make_batch(spec, 3, 5)[0]
    b.set_act_path("image")
    b.qvalues(obs)
    for k in ("h1", "q"):
        with pytest.raises(B.BdrError, match="image path"):
            b.probe(k, 3)
    b.close()
    g = B.CandleDqnCnnGroup([a, c])
    with pytest.raises(B.BdrError, match="member of a group"):
        c.set_head_form("splitk")
    g.close()
