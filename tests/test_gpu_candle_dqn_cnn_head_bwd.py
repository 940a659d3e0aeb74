"""set_head_bwd_form("fused") of the candle DQN's AtariCnn form: l2's and l1's input gradients and the head's weight gradients in one
launch, k_cdqn_head_bwd (csrc/cdqn_head_bwd.hpp).  The head's four gradient segments and c3.bias's are checked against float64 formed
from the device's own a3, h1 and dpred (tests/dqn_backward_reference.py: its Op, its three criteria, u = 2^-24); the conv
segments against a "layers" twin under the same bound with S from the float64 chain.  All of it fails without the entry point.
Lambda is 1.0 for every segment but l1.weight.  There criterion (c) fails at 1.0 at B = 3 alone (142 of 1 605 632 elements above
sqrt(3) u S, the largest 1.358: three terms added in sequence may err by 3 u S, criterion (b), which holds); that file's own sequential
float32 restatement reaches 1.343 there, and its table entry for the output, LAMBDA["gW4"] = max(1, 4 x 1.343) = 5.37, is used."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import candle_dqn_cnn_restatement as R  # noqa: E402
import candle_dqn_restatement as RM  # noqa: E402
import dqn_backward_reference as G  # noqa: E402
from dqn_forward_reference import unflat  # noqa: E402

pytestmark = pytest.mark.gpu
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
# (B, n_stack, A, double_dqn): one row; three instances and 18 actions; a ragged second row tile; three row tiles, the last ragged
UPDATES = ((1, 4, 6, False), (3, 1, 18, True), (33, 4, 2, False), (65, 4, 6, False))
HEAD = {"l1.weight": "gW4", "l1.bias": "gb4", "l2.weight": "gW5", "l2.bias": "gb5"}   # the reference's names of the head segments
CONV = {"c1.weight": "gW1", "c1.bias": "gb1", "c2.weight": "gW2", "c2.bias": "gb2", "c3.weight": "gW3", "c3.bias": "gb3"}
NAMES = ["sample", "fwd_conv", "fwd_conv", "fwd_conv", "fwd", "fwd", "cdqn_td", "bwd_head", "reduce_adam",
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


def agent(B, spec, params, bsz, bwd="fused", head="layers"):
    a = B.CandleDqn.build(spec.to_config(B, bsz, device=0))
    a.set_head_form(head)
    a.set_head_bwd_form(bwd)
    a.set_params(params[0], "qnet"); a.set_params(params[1], "qnet_tgt")
    return a


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def float64_chain(a, params, batch, Bn, ns, A):
    """dqn_backward_reference's Ops of the whole backward from the device's a1, a2, a3, h1 and dpred.  dh1 is one product per element
    (dq is one-hot): dy[0] holds it rounded to f32 and the chain goes on from that, as the kernel does; dy3, dy2, dy1 stay float64."""
    inp = dict(params=unflat(params[0], R.var_shapes(ns, A)), obs=batch[0], act=batch[1], dq=a.probe("dpred", Bn),
               **{k: a.probe(k, Bn) for k in ("a1", "a2", "a3", "h1")})
    stages = dict(dh1="h1", dy3="a3", dy2="a2", dy1="a1")   # each gradient has the shape of the activation beside it
    inp.update({k: np.zeros(inp[like].shape) for k, like in stages.items()})
    for k in stages:                                        # in chain order: each stage reads the ones before it
        inp[k] = G.reference(inp, only=(k,))[k].ref.astype(np.float32 if k == "dh1" else np.float64)
    ops = G.reference(inp, only=("dy3",) + tuple(HEAD.values()) + tuple(CONV.values()))
    # c3.bias as the plain sum of the float64 dy3: the device adds its own dy3, each element 512 terms, over B * 49 positions
    dy3 = ops["dy3"]
    ops["gb3"] = G.Op("gb3", dy3.ref.sum((0, 1, 2)), dy3.S.sum((0, 1, 2)), np.full(64, Bn * 49 * 512.0), kern="k_cdqn_head_bwd (dy3) + conv3 dW")
    return ops


@pytest.mark.parametrize("Bn,ns,A,double", UPDATES)
def test_head_gradients_against_float64(B, Bn, ns, A, double):
    """largest |err| / (sqrt(n) u S) measured over the four cases: l1.weight 1.358 (B = 3), l1.bias 0.695,
    l2.weight 0.962, l2.bias 0.252, c3.bias 0.002; every conv segment bit-equal to the twin's"""
    spec, params, batch = case(Bn, ns, A, double)
    a, twin = agent(B, spec, params, Bn), agent(B, spec, params, Bn, "layers")
    a.update_on_batch(*batch); twin.update_on_batch(*batch)
    ops = float64_chain(a, params, batch, Bn, ns, A)
    g, gt = (dict(zip(R.VAR_NAMES, unflat(x.get_params("qnet", "grad"), R.var_shapes(ns, A)))) for x in (a, twin))
    v = {name: G.check(ops[k], g[name], G.LAMBDA[k] if k == "gW4" else 1.0) for name, k in dict(HEAD, **{"c3.bias": "gb3"}).items()}
    # the conv segments against the layer form: the same bound, S and n from the float64 chain, the twin's value in the reference's place
    vt = {name: G.check(G.Op(k, gt[name].astype(np.float64), ops[k].S, ops[k].n, kern="conv backward behind k_cdqn_head_bwd"), g[name], 1.0)
          for name, k in CONV.items()}
    print("f64", {name: round(x.sharp_ratio, 3) for name, x in v.items()}, "twin", {name: round(x.sharp_ratio, 3) for name, x in vt.items()})
    bad = [x.message for x in list(v.values()) + list(vt.values()) if not x.ok]
    assert not bad, "\n".join(bad)
    assert all(g[name].any() for name in HEAD)
    # up to 16 rows both forms add a batch in one accumulator, row by row (one row: nothing is added at all); from 17 rows up the layer
    # form splits the rows over four waves and the fused form does not: there the bits must differ somewhere
    assert Bn <= 16 or any((bits(g[name]) != bits(gt[name])).any() for name in HEAD)
    a.close(); twin.close()


def test_the_rest_of_the_update_is_untouched(B):
    spec, params, batch = case(*UPDATES[2])
    a = agent(B, spec, params, 33)
    a.update_on_batch(*batch); a.update_on_batch(*batch)
    fresh = agent(B, spec, (a.get_params("qnet"), a.get_params("qnet_tgt")), 33)
    a.update_on_batch(*batch); fresh.update_on_batch(*batch)
    for k in ("pred", "q_next", "tgt"):
        assert (bits(a.probe(k, 33)) == bits(fresh.probe(k, 33))).all(), k
    a.close(); fresh.close()


def test_above_the_batch_limit_the_layer_launches_run(B):
    (spec, params, batch), Bn = case(257, 1, 2, False), 257   # CHB_MAX_B + 1
    a, twin = agent(B, spec, params, Bn), agent(B, spec, params, Bn, "layers")
    a.update_on_batch(*batch); twin.update_on_batch(*batch)
    for which in (("qnet", "grad"), ("qnet",), ("qnet_tgt",), ("qnet", "exp_avg"), ("qnet", "exp_avg_sq")):
        assert (bits(a.get_params(*which)) == bits(twin.get_params(*which))).all(), which
    a.close(); twin.close()


@pytest.mark.parametrize("head", ("layers", "splitk"))
def test_one_bwd_head_where_dx_dx_dw_stood(B, head):
    spec, params, batch = case(3, 4, 6, False)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=1), (spec.row_bytes,), np.uint8, (1,), np.int64)
    rb.push(batch[0], batch[1].reshape(-1, 1), *batch[2:])

    def names(a):
        a.opt(rb); a.profile_enable(True); a.opt(rb); a.sync()
        got = [k for k, _ in a.profile_read()]
        a.profile_enable(False)
        return got
    want = NAMES if head == "layers" else NAMES[:4] + ["fwd_head"] + NAMES[6:]
    a, back = agent(B, spec, params, 3, head=head), agent(B, spec, params, 3, head=head)
    assert names(a) == want, names(a)
    back.opt(rb); back.set_head_bwd_form("layers")    # the way back: the layer form's list, as it always was
    k = want.index("bwd_head")
    assert names(back) == want[:k] + ["dx", "dx", "dw"] + want[k + 1:]
    a.close(); back.close(); rb.close()


def test_what_the_switch_and_the_group_rule_refuse(B):
    spec, params, _ = case(3, 4, 6, False)
    a, b, c = agent(B, spec, params, 3, "layers"), agent(B, spec, params, 3), agent(B, spec, params, 3, "layers")
    for value in (-1, 2):
        assert B._lib.lib().bdr_candle_dqn_cnn_set_head_bwd_form(a.handle, value) == 1 and b"unknown head backward form" in B._lib.lib().bdr_last_error()
    with pytest.raises(B.BdrError, match="BDR_HEAD_BWD_FUSED"):
        B.CandleDqnCnnGroup([a, b])
    mlp = B.CandleDqn.build(RM.CandleDqnSpec(5, 4, (32,), adamw=ADAMW).to_config(B, 2, device=0))
    with pytest.raises(B.BdrError, match="AtariCnn"):
        mlp.set_head_bwd_form("fused")
    wide = B.CandleDqn.build(R.CandleDqnCnnSpec(4, 33, adamw=ADAMW).to_config(B, 2, device=0))
    with pytest.raises(B.BdrError, match="at most 32 actions"):
        wide.set_head_bwd_form("fused")
    mlp.close(); b.close(); wide.close()
    g = B.CandleDqnCnnGroup([a, c])
    with pytest.raises(B.BdrError, match="member of a group"):
        c.set_head_bwd_form("fused")
    g.close()
