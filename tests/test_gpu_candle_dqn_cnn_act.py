"""BDR_ACT_PATH_IMAGE, the two-launch acting path of the candle DQN's AtariCnn form (csrc/cnn_act_img.hpp), against the float32 and
float64 forward of tests/candle_dqn_cnn_restatement.py.

Bar: 4 x the largest |float32 restatement - float64 restatement| over the Q values of the very same parameters and
frames, with torch on one thread; the device is held to |Q_device - Q_float64| <= bar, and its greedy action to the float64 argmax on
every row whose top-two gap exceeds 2 x the bar - the seeds are such that this is every row.  conv2's ragged tile (81 = 64 + 17
positions) and conv3's (49 = 32 + 17) are in every image."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import bc_restatement as RB  # noqa: E402
import candle_dqn_cnn_restatement as R  # noqa: E402
import candle_dqn_restatement as RM  # noqa: E402

pytestmark = pytest.mark.gpu
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
SHAPES = ((1, 2), (4, 6), (4, 18))     # (n_stack, actions): the network's shapes
ROWS = (1, 3, 32)                      # one row, ragged, the full tile
CASES = [(s, n, "host") for s in SHAPES for n in ROWS] + [((4, 6), 3, "dense"), ((4, 6), 3, "strided")]


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


@functools.lru_cache(maxsize=None)
@R.single_thread
def reference(n_stack, A, n):
    """spec, parameters, n frame stacks, the float64 Q rows and the bar - once per session"""
    spec = R.CandleDqnCnnSpec(n_stack, A, adamw=ADAMW)
    p = spec.init_params(100 * n_stack + A)[0]
    obs = R.make_batch(spec, n, 7 * n + A)[0]
    q32 = R.CandleDqnCnnRestatement(spec, p, p, torch.float32).qvalues(obs.astype(np.float32)).astype(np.float64)
    q64 = R.CandleDqnCnnRestatement(spec, p, p, torch.float64).qvalues(obs.astype(np.float32)).astype(np.float64)
    return spec, p, obs, q64, 4.0 * float(np.abs(q32 - q64).max())


def agent(B, spec, p, bsz, path="image", **kw):
    a = B.CandleDqn.build(spec.to_config(B, bsz, device=0, **kw))
    a.set_params(p, "qnet"); a.set_params(p, "qnet_tgt")
    a.set_act_path(path)
    return a


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape,n,rows", CASES)
def test_q_and_the_greedy_action_against_float64(B, shape, n, rows):
    spec, p, obs, q64, bar = reference(*shape, n)
    top = np.sort(q64, axis=1)
    assert (top[:, -1] - top[:, -2]).min() > 2 * bar, "the seeds leave no row out of the greedy comparison"
    assert RM.CandleDqnExplorer(seed=1).rng.gen_f32() >= np.float32(0.01)   # eval mode, seed 1: the first call is a greedy one
    a = agent(B, spec, p, n)
    a.set_explorer(B.Softmax(), seed=1)
    if rows == "host":
        q, act = a.qvalues(obs), a.sample(obs)
    else:
        pad = 0 if rows == "dense" else 8
        dev = torch.zeros((n, spec.row_bytes + pad), dtype=torch.uint8, device="cuda")
        dev[:, :spec.row_bytes] = torch.from_numpy(obs).cuda()
        torch.cuda.synchronize()
        q = a.qvalues_device(dev.data_ptr(), n, spec.row_bytes + pad)
        act = a.sample_device(dev.data_ptr(), n, spec.row_bytes + pad)
    d = float(np.abs(q.astype(np.float64) - q64).max())
    print(shape, n, rows, "|q - q64|", d, "bar", bar)
    assert q.shape == (n, shape[1]) and d <= bar
    assert (act == q64.argmax(1)).all()   # the device's own first maximum (samp_idx)
    a.close()


def test_33_rows_take_the_layer_launches_bit_for_bit(B):
    spec, p, _, _, _ = reference(4, 6, 3)
    obs = R.make_batch(spec, 33, 5)[0]
    a, b = agent(B, spec, p, 33), agent(B, spec, p, 33, "layers")
    assert (bits(a.qvalues(obs)) == bits(b.qvalues(obs))).all()
    assert (a.sample_greedy(obs) == b.sample_greedy(obs)).all()
    assert not (bits(a.qvalues(obs[:32])) == bits(b.qvalues(obs[:32]))).all()   # 32 rows do take the other path: another order of the sums
    a.close(); b.close()


@pytest.mark.parametrize("n", (1, 3))
def test_the_explorers_read_the_paths_own_q_and_advance_the_stream_as_the_layer_path_does(B, n):
    spec, p, obs, q64, bar = reference(4, 6, n)
    eg = dict(train=True, explorer=B.EpsilonGreedy(eps_start=1.0, eps_final=0.02, final_step=50))
    a, twin = agent(B, spec, p, n, **eg), agent(B, spec, p, n, "layers", **eg)
    q = a.qvalues(obs)
    assert (q.argmax(1) == twin.qvalues(obs).argmax(1)).all()
    ex = RM.CandleDqnExplorer("eps_greedy", 1.0, 0.02, 50, seed=42)
    for i in range(80):   # random and greedy calls: the same draws in both agents
        got = a.sample(obs)
        assert (got == ex.sample(q, True)).all() and (got == twin.sample(obs)).all(), i
    a.set_explorer(B.Softmax(), seed=7)
    ex = RM.CandleDqnExplorer("softmax", seed=7)
    for i in range(40):
        assert (a.sample(obs) == ex.sample(q, True)).all(), i
    a.close(); twin.close()


def test_one_acting_call_is_the_trunk_and_the_head(B):
    spec, p, obs, _, _ = reference(4, 6, 3)
    a = agent(B, spec, p, 3)
    a.qvalues(obs)
    a.profile_enable(True)
    a.qvalues(obs)
    names = [k for k, _ in a.profile_read()]
    a.profile_enable(False)
    assert names == ["act_trunk", "act_head"], names
    a.close()


def test_refusals(B):
    mlp = RM.CandleDqnSpec(5, 4, (32,), adamw=ADAMW)
    m = B.CandleDqn.build(mlp.to_config(B, 2, device=0))
    bc = B.Bc.build(RB.BcSpec(5, 3, (32,)).to_config(B, 4, device=0, seed=1))
    for x in (m, bc):
        with pytest.raises(B.BdrError, match="BDR_ACT_PATH_IMAGE"):
            x.set_act_path("image")
        x.close()
    spec, p, _, _, _ = reference(1, 2, 1)
    a = agent(B, spec, p, 1)
    with pytest.raises(B.BdrError, match="fused acting kernel"):
        a.set_act_path("fused")
    a.close()
