"""conv3's input gradient as the step launches it (k_igemm<DxC3PosL, 2, PEEL>: ADxS1PosLean's tap addressing, the k loop's last step
peeled so that the loop carries no team test) against the form before it (k_igemm<DxC3Pos, 2>, BDR_DXC3_KLOOP=0) and against f64.

Both forms load the same values and feed every accumulator the same products in the same order - team 0 the channels 0..31 of every
valid tap, team 1 the channels 32..63, the two added once at the end - so dy2 and everything behind it must agree word for word.
Every launch walks all 81 input positions, i.e. every loop length the kernel has (1, 2, 3, 4, 6 and 9 taps: odd and even, and the
1-tap corners where only the peeled step runs).  Batch sizes: 1 (one valid row in a 64-row tile: 63 padding rows on the zero-stride
addresses), 64 (exactly one tile), 65 (a second tile with one row), 40 (tests/test_gpu_dqn_backward.py's partial-buffer case).  The
switch is read when an agent is constructed, so the two agents of a comparison live side by side.
Measured on an MI355X: 0 differing words in every case; dy2 against f64 at B = 40: largest |err| / (sqrt(n) u S) 0.261 (lambda 1.61)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dqn_backward_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
A, NS = 6, 4


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def make_agent(B, monkeypatch, Bsz, kloop):
    """kloop: False -> BDR_DXC3_KLOOP=0 (the form before), True -> the default"""
    monkeypatch.delenv("BDR_SCHED", raising=False); monkeypatch.delenv("BDR_DQN_F32_EXACT", raising=False)
    if kloop: monkeypatch.delenv("BDR_DXC3_KLOOP", raising=False)
    else: monkeypatch.setenv("BDR_DXC3_KLOOP", "0")
    cfg = B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.AtariCnnConfig(n_stack=NS, out_dim=A), opt_config=B.OptimizerConfig.Adam(1e-4)),
                      device=0, batch_size=Bsz, critic_loss="SmoothL1", tau=1.0, soft_update_interval=10000, double_dqn=False)
    a = B.Dqn.build(cfg)
    p0, _ = R.case_params(A, NS, 100 + Bsz)
    a.set_params(p0, "qnet"); a.set_params(p0, "qnet_tgt")
    return a


def test_the_positions_cover_every_loop_length():
    counts = {R.taps_c3(i) * R.taps_c3(j) for i in range(9) for j in range(9)}
    assert counts == {1, 2, 3, 4, 6, 9}


@pytest.mark.parametrize("Bsz", [1, 64, 65, 40])
def test_same_bits_as_the_form_before(B, monkeypatch, Bsz):
    counts = np.array([[R.taps_c3(i) * R.taps_c3(j) for j in range(9)] for i in range(9)])
    assert set(counts.ravel().tolist()) == {1, 2, 3, 4, 6, 9}, "a launch must walk every loop length"
    old, new = make_agent(B, monkeypatch, Bsz, False), make_agent(B, monkeypatch, Bsz, True)
    try:
        first, second = R.case_batch(Bsz, A, NS, 200 + Bsz), R.case_batch(Bsz, A, NS, 300 + Bsz)
        for a in (old, new): a.update_on_batch(*first)
        d_old, d_new = (a.probe("dy2", Bsz * 81 * 64).reshape(Bsz, 9, 9, 64) for a in (old, new))
        for n in (1, 2, 3, 4, 6, 9):   # not a vacuous comparison: every tap class has non-zero gradients
            assert (d_new[:, counts == n] != 0).any(), "no gradient at the %d-tap positions" % n
        assert np.array_equal(bits(d_old), bits(d_new)), "dy2 differs in %d words" % (bits(d_old) != bits(d_new)).sum()
        for a in (old, new): a.update_on_batch(*second)
        for k in ("qnet", "exp_avg"):
            assert np.array_equal(bits(old.get_params(k)), bits(new.get_params(k))), k
        assert not np.array_equal(bits(new.get_params("qnet")), bits(R.case_params(A, NS, 100 + Bsz)[0])), "the updates moved nothing"
    finally:
        old.close(); new.close()


def test_dy2_against_f64(B, monkeypatch):
    """dqn_backward_reference's bound, element by element (u = 2^-24, S = sum |a||b|; (a), (b) and (c) of its check), no element exempt"""
    from oracle import torch_ref as T
    Bsz = 40
    a = make_agent(B, monkeypatch, Bsz, True)
    try:
        p0, shapes = R.case_params(A, NS, 100 + Bsz)
        params = [t.detach().numpy() for t in T.unflatten(p0, shapes)]
        obs, act, nobs, rew, term = R.case_batch(Bsz, A, NS, 200 + Bsz)
        a.update_on_batch(obs, act, nobs, rew, term)
        n = Bsz
        inp = dict(params=params, obs=obs, act=act,
                   a1=a.probe("act_conv1", n * 400 * 32).reshape(n, 20, 20, 32), a2=a.probe("act_conv2", n * 81 * 64).reshape(n, 9, 9, 64),
                   a3=a.probe("act_conv3", n * 49 * 64).reshape(n, 7, 7, 64), h1=a.probe("h1", n * 512).reshape(n, 512), dq=a.probe("dq", n),
                   dh1=a.probe("dh1", n * 512).reshape(n, 512), dy3=a.probe("dy3", n * 49 * 64).reshape(n, 7, 7, 64),
                   dy2=a.probe("dy2", n * 81 * 64).reshape(n, 9, 9, 64), dy1=a.probe("dy1", n * 400 * 32).reshape(n, 20, 20, 32))
        assert np.abs(inp["dy3"]).max() > 0 and (inp["a2"] > 0).any(), "a vacuous case"
        ops = R.reference(inp, only=("dy2",))
        dev = {"dy2": inp["dy2"]}
        print("dy2 ratio, lean addressing + peeled loop, B=40: %.3f (lambda %.2f)" % (R.sharp_ratios(ops, dev)["dy2"], R.LAMBDA["dy2"]))
        R.check_all(ops, dev, R.LAMBDA)
    finally:
        a.close()


def test_the_shared_trunk_takes_the_same_step(B, monkeypatch):
    """the candle DQN's AtariCnn Q-network reaches the launch through conv_trunk.hpp: one update at a small batch, switch at 0 and
    at the default - gradients, moments, parameters and target parameters bit for bit"""
    import candle_dqn_cnn_restatement as C
    spec = C.CandleDqnCnnSpec(4, 6, lr=1e-4, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01), double_dqn=True)
    params, batch = spec.init_params(77), C.make_batch(spec, 5, 78)
    agents = []
    try:
        for kloop in (False, True):
            if kloop: monkeypatch.delenv("BDR_DXC3_KLOOP", raising=False)
            else: monkeypatch.setenv("BDR_DXC3_KLOOP", "0")
            a = B.CandleDqn.build(spec.to_config(B, 5, device=0))
            agents.append(a)
            a.set_params(params[0], "qnet"); a.set_params(params[1], "qnet_tgt")
            a.update_on_batch(*batch)
        old, new = agents
        assert np.abs(new.get_params("qnet", "grad")).max() > 0
        assert not np.array_equal(bits(new.get_params("qnet")), bits(params[0]))
        for k in ("qnet", "qnet_tgt"):
            assert np.array_equal(bits(old.get_params(k)), bits(new.get_params(k))), k
        for role in ("grad", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(bits(old.get_params("qnet", role)), bits(new.get_params("qnet", role))), role
    finally:
        for a in agents: a.close()
