"""Every kernel of the CNN DQN step's backward pass against an f64 evaluation of ITS OWN layer on the device's own inputs.

The end-to-end gradient checks of tests/test_gpu_dqn.py (assert_grads_close: 2e-4 of a variable's largest entry, two exempt
channels) sit about 1000 x above what these kernels can produce: every product in them is exact and only the f32 accumulation
rounds.  Here each kernel's output - dh1 (TD part of k_head), the l2 gradients (k_head_bwd), l1 / conv3 / conv2 weight gradients
(k_igemm_red<DwL1 / DwC3 / DwC2>), the input gradients dy3 / dy2 / dy1 (launch_igemm<DxL1 / DxC3Pos / DxC2MPos>), conv1's weight
gradient (launch_conv1_dw_bf16) and, for the conv layers, the partial-sum reduction of k_reduce_adam behind them - is compared with
tests/dqn_backward_reference.py: parameters as set before the step, activations / h1 / dq / dh1 / dy* from Dqn.probe, ReLU masks from the
probed activations, so NO element is exempt.  Per element, u = 2^-24, S = sum |a_k| |b_k|, n the reduction length:
  (a) S == 0 -> exactly 0;   (b) |err| <= n u S;   (c) |err| <= lambda sqrt(n) u S, lambda = 4 x the sequential f32 restatement's
largest ratio on these cases' inputs, floored at 1 (dqn_backward_reference.LAMBDA; not fitted to the device).

Largest |err| / (sqrt(n) u S) over the cases below, sequential f32 restatement on the CPU | measured on an MI355X (the largest of
the "backward ratios" lines that the tests print: all cases, both schedules, both arithmetics, follow-up updates and the overlapped
opt steps included) | lambda.  The device sits a factor 3 or more below lambda everywhere; its largest figures (dh1, the head and l1
gradients) are those of the short sums, where one rounding is most of the error and (b) binds.  If a later change fails (c) by a
small factor, compare its printed line with this record first:
  dh1  k_head (TD part)       restatement 0.999 | MI355X 0.997 | lambda 4.00
  gW5  k_head_bwd             restatement 1.396 | MI355X 1.543 | lambda 5.58
  gb5  k_head_bwd             restatement 0.649 | MI355X 0.811 | lambda 2.60
  gW4  k_igemm_red<DwL1>      restatement 1.343 | MI355X 1.614 | lambda 5.37
  gb4  k_igemm_red<DwL1>      restatement 1.016 | MI355X 0.850 | lambda 4.06
  dy3  launch_igemm<DxL1>     restatement 0.202 | MI355X 0.135 | lambda 1.00
  gW3  k_igemm_red<DwC3>      restatement 0.444 | MI355X 0.327 | lambda 1.78
  gb3  k_igemm_red<DwC3>      restatement 0.190 | MI355X 0.114 | lambda 1.00
  dy2  launch_igemm<DxC3Pos>  restatement 0.402 | MI355X 0.301 | lambda 1.61
  gW2  k_igemm_red<DwC2>      restatement 0.466 | MI355X 0.320 | lambda 1.86
  gb2  k_igemm_red<DwC2>      restatement 0.163 | MI355X 0.083 | lambda 1.00
  dy1  launch_igemm<DxC2MPos> restatement 0.448 | MI355X 0.510 | lambda 1.79
  gW1  launch_conv1_dw_bf16   restatement 0.212 | MI355X 0.155 | lambda 1.00
  gb1  launch_conv1_dw_bf16   restatement 0.080 | MI355X 0.020 | lambda 1.00

Cases (B, A, n_stack): (1, 6, 4) tiles almost all padding, one conv1-dW workgroup; (3, 9, 1) idle conv1-dW waves, 24-action head
block; (7, 4, 8) two conv1-dW row tiles per wave; (40, 6, 4) both chunk caps reached with uneven tiles per chunk (conv2: 102 row
tiles over 64 chunks, conv3: 62 over 56); (65, 18, 4, double DQN) the second 64-image tile of the position-class kernels and of
DxL1 holds one image; (257, 33, 4) k_head_bwd's second 256-row pass holds one row, conv1-dW workgroups take two images, 64-action
head block.  Actions (dqn_backward_reference.head_bwd_actions): action 0 has no rows, action 1 has 17 or more from B = 24 on (here:
B = 40, 65 and 257; a smaller batch cannot hold them), the others a few each.  On the B = 65 agent a B = 5 update follows (capacity >
batch: the partial-buffer layout follows the capacity; neither stale chunks nor rows beyond M may enter), on the B = 40 agent a second update at once (update_on_batch returns with both
queues joined, so the two do not overlap in time; what carries over - the partials, dy*, the a1 buffers - is what is checked).
B = 40 and 65 also run with BDR_SCHED=0 (one queue), B = 40 once with arithmetic="f32_exact"."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_backward_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def make_agent(B, Bsz, A, ns, ddqn, **kw):
    cfg = B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.AtariCnnConfig(n_stack=ns, out_dim=A), opt_config=B.OptimizerConfig.Adam(1e-4)),
                      device=0, batch_size=Bsz, critic_loss="SmoothL1", tau=1.0, soft_update_interval=10000, double_dqn=ddqn, **kw)
    return B.Dqn.build(cfg)


def update_and_check(a, shapes, batch, label):
    """One update_on_batch, then every backward output against the reference on the probed inputs.  Prints the device's ratios."""
    from oracle import torch_ref as T
    obs, act, nobs, rew, term = batch
    params = [t.detach().numpy() for t in T.unflatten(a.get_params("qnet"), shapes)]     # BEFORE the optimizer step
    a.update_on_batch(obs, act, nobs, rew, term)
    inp = probed_inputs(a, params, obs, act)
    assert np.abs(inp["dq"]).max() > 0 and all((inp[k] > 0).any() for k in ("a1", "a2", "a3", "h1")), "a vacuous case"
    grads = [t.detach().numpy() for t in T.unflatten(a.get_params("grad"), shapes)]
    dev = {k: inp[k] for k in ("dh1", "dy3", "dy2", "dy1")}
    dev.update({k: grads[i] for k, i in R.GRAD_INDEX.items()})
    ops = R.reference(inp)
    ratios = R.sharp_ratios(ops, dev)
    print("backward ratios %s: " % label + " ".join("%s %.3f" % (k, ratios[k]) for k in R.OPS))
    R.check_all(ops, dev, R.LAMBDA)


def probed_inputs(a, params, obs, act):
    n = len(act)
    return dict(params=params, obs=obs, act=act,
                a1=a.probe("act_conv1", n * 400 * 32).reshape(n, 20, 20, 32), a2=a.probe("act_conv2", n * 81 * 64).reshape(n, 9, 9, 64),
                a3=a.probe("act_conv3", n * 49 * 64).reshape(n, 7, 7, 64), h1=a.probe("h1", n * 512).reshape(n, 512), dq=a.probe("dq", n),
                dh1=a.probe("dh1", n * 512).reshape(n, 512), dy3=a.probe("dy3", n * 49 * 64).reshape(n, 7, 7, 64),
                dy2=a.probe("dy2", n * 81 * 64).reshape(n, 9, 9, 64), dy1=a.probe("dy1", n * 400 * 32).reshape(n, 20, 20, 32))


def run_case(B, Bsz, A, ns, ddqn, label, follow_up=None, **kw):
    p0, shapes = R.case_params(A, ns, 100 + Bsz)
    a = make_agent(B, Bsz, A, ns, ddqn, **kw)
    try:
        a.set_params(p0, "qnet"); a.set_params(p0, "qnet_tgt")
        update_and_check(a, shapes, R.case_batch(Bsz, A, ns, 200 + Bsz), label)
        if follow_up:
            update_and_check(a, shapes, R.case_batch(follow_up, A, ns, 300 + follow_up), label + " then B=%d" % follow_up)
    finally:
        a.close()


FOLLOW_UP = {40: 40, 65: 5}   # B = 40: a second update at once; B = 65: a smaller batch in the larger agent's buffers


@pytest.mark.parametrize("Bsz,A,ns,ddqn", R.CASES, ids=["B%d-A%d-ns%d%s" % (b, a, ns, "-ddqn" if d else "") for b, a, ns, d in R.CASES])
def test_backward_kernels_layer_by_layer(B, monkeypatch, Bsz, A, ns, ddqn):
    monkeypatch.delenv("BDR_SCHED", raising=False); monkeypatch.delenv("BDR_DQN_F32_EXACT", raising=False)
    run_case(B, Bsz, A, ns, ddqn, "B=%d A=%d ns=%d" % (Bsz, A, ns), follow_up=FOLLOW_UP.get(Bsz))


@pytest.mark.parametrize("Bsz,A,ns,ddqn", [c for c in R.CASES if c[0] in (40, 65)], ids=["B40", "B65-ddqn"])
def test_backward_kernels_layer_by_layer_on_one_queue(B, monkeypatch, Bsz, A, ns, ddqn):
    monkeypatch.setenv("BDR_SCHED", "0"); monkeypatch.delenv("BDR_DQN_F32_EXACT", raising=False)
    run_case(B, Bsz, A, ns, ddqn, "B=%d A=%d ns=%d BDR_SCHED=0" % (Bsz, A, ns), follow_up=FOLLOW_UP.get(Bsz))


def test_backward_kernels_layer_by_layer_with_the_exact_forward(B, monkeypatch):
    monkeypatch.delenv("BDR_SCHED", raising=False); monkeypatch.delenv("BDR_DQN_F32_EXACT", raising=False)
    run_case(B, 40, 6, 4, False, "B=40 A=6 ns=4 f32_exact", follow_up=40, arithmetic="f32_exact")


def test_weight_gradients_of_opt_steps_that_overlap(B, monkeypatch):
    """Three Agent::opt calls over a replay ring with nothing between them: with the overlapped tail conv2 dW and the conv2 / conv3
    optimizer pass of one step run on the other queue while the next step's conv1 forward writes the OTHER a1 buffer.  The probes go
    behind that queue's flag and return the buffers the LAST step's kernels read (act_conv1: the one its conv2 dW read), so every
    weight gradient of the last step is checked as above.  (The dX kernels need the parameters in front of the last step, which
    nothing can read without joining the queues between the steps; they are covered by the update_on_batch cases.)"""
    from oracle import oracle as O
    from oracle import torch_ref as T
    from tests import synth
    monkeypatch.delenv("BDR_SCHED", raising=False); monkeypatch.delenv("BDR_DQN_F32_EXACT", raising=False)
    cap, Bsz, A = 256, 40, 6
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=42), (4, 1, 84, 84), np.uint8)
    rb.fill_synthetic(cap, seed=3, kind=0, n_actions=A)
    rows = synth.atari_rows(3, 0, cap)
    oref = O.Replay(cap, 42, 28224, 8)
    oref.push(rows[0], rows[1].reshape(-1, 1), rows[2], rows[3], rows[4], rows[5])
    p0, shapes = R.case_params(A, 4, 140)
    a = make_agent(B, Bsz, A, 4, False)
    try:
        a.set_params(p0, "qnet"); a.set_params(p0, "qnet_tgt")
        for _ in range(3):
            a.opt(rb)
            b = oref.batch(Bsz)
        obs, act = b["obs"].reshape(Bsz, 4, 1, 84, 84), b["act"].view(np.int64).ravel()
        # p0 is stale after three Adam steps: only the outputs that read no parameter are evaluated (only=), never the dX ones
        inp = probed_inputs(a, [t.detach().numpy() for t in T.unflatten(p0, shapes)], obs, act)
        grads = [t.detach().numpy() for t in T.unflatten(a.get_params("grad"), shapes)]
        assert np.abs(inp["dq"]).max() > 0
        dev = {k: grads[i] for k, i in R.GRAD_INDEX.items()}
        ops = R.reference(inp, only=tuple(R.GRAD_INDEX))
        assert set(ops) == set(dev) == set(R.GRAD_INDEX)
        print("backward ratios opt x 3, B=40: " + " ".join("%s %.3f" % kv for kv in R.sharp_ratios(ops, dev).items()))
        R.check_all(ops, dev, R.LAMBDA)
    finally:
        a.close(); rb.close()
