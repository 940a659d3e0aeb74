"""Every kernel of the CNN DQN step's forward pass against an f64 evaluation of ITS OWN layer on the device's own input of that layer.

The end-to-end checks of tests/test_gpu_dqn.py see the forward through Q values at 1e-5 or looser, and its per-layer budget is 1e-6 of
a layer's LARGEST output.  Here a1 (k_conv1_bf16<NS> / k_conv1_bf16_img<NS, IPW, NT>), a2 and a3 (k_fwd_c23_b3, FwdC2B3 / FwdC3B3, the
FP32-MFMA forms, k_act_layer<2> / <3>), h1 (FwdL1X + k_head, k_act_layer<0>) and the Q rows (k_head's l2, the acting head) of EVERY
network instance that ran - slot 0 qnet(obs), slot 1 qnet_tgt(next_obs), slot 2 qnet(next_obs) with double DQN, through probes 14-22 -
are compared element by element with tests/dqn_forward_reference.py: a1 from the u8 rows, a2 from the probed a1, a3 from the probed
a2, h1 from the probed a3, q from the probed h1, parameters as set (qnet and qnet_tgt differ, so an instance that read the other set's
weights or planes fails).  Per element, u = 2^-24, S = sum |a_k| |b_k| + |bias|, n = K + 1:
  (a) S == 0 -> exactly 0;   (b) |err| <= n u S;   (c) |err| <= lambda sqrt(n) u S, lambda = 4 x the sequential f32 restatement's
largest ratio, floored at 1 (dqn_forward_reference.LAMBDA; not fitted to the device); the split arithmetic's three dropped products
(SPLIT_C * S) and conv1's 1/255 rounding are taken off first.  No element is exempt.

Largest |err| / (sqrt(n) u S) over everything below, sequential f32 restatement on the CPU | measured on an MI355X (the largest of the
"forward ratios" lines that the tests print; a record, not a bar) | lambda.  The device sits a factor 4.8 or more below lambda everywhere
and at or below the sequential restatement (MFMA steps, k-slices and butterflies sum in trees).  Of the split forms the fused kernel and
the two launches print the same figures (they are bit-identical); the largest a2 is the exact FP32-MFMA form's at B = 256
(tests/test_gpu_dqn.py's per-layer budget test prints it; the split forms' largest is 0.204, at B = 257), the largest a3 the split form's at n = 24 acting rows; the
acting kernels (n <= 8) stay below 0.05 on a2 / a3.  If a later change fails (c) by a small
factor, compare its printed line with this record first:
  a1  conv1 (both forms, acting)         restatement 0.338 | MI355X 0.188 | lambda 1.35
  a2  conv2 (fused, two-launch, exact)   restatement 0.263 | MI355X 0.217 | lambda 1.05
  a3  conv3 (fused, two-launch, exact)   restatement 0.189 | MI355X 0.193 | lambda 1.00
  h1  FwdL1X + k_head / k_act_layer<0>   restatement 0.052 | MI355X 0.019 | lambda 1.00
  q   k_head l2 / acting head            restatement 0.059 | MI355X 0.032 | lambda 1.00

Cases (B, A, n_stack): (1, 6, 4) every tile almost all padding, the fused conv2+conv3 kernel with one image; (3, 9, 1) the 24-action
head; (7, 4, 8) the direct conv1 form, an all-zero and an all-255 image; (40, 6, 4) M = 3240 and 1960: a ragged last 128-row tile of the
two-launch form, the edge images again; (65, 18, 4, double DQN) three instances in one launch, the second 64-row l1 tile holds one row;
(257, 33, 4) two images per conv1 pass with the last pass holding one, the 64-action head, the HEAD_ROWS tail.  B = 40 and 65 also run
with BDR_SCHED=0, with the per-kernel profile on (one launch per layer: the labels say so) and with arithmetic="f32_exact"; one run
goes through opt() over a ring, where slot 1 comes from the other queue's split target forward."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_forward_reference as Fw  # noqa: E402

pytestmark = pytest.mark.gpu

LAYERS = ("a1", "a2", "a3", "h1")
# probe names of (a1, a2, a3, h1, q) per instance slot
PROBES = {0: ("act_conv1", "act_conv2", "act_conv3", "h1", "q_pred_all"), 1: ("tgt_conv1", "tgt_conv2", "tgt_conv3", "tgt_h1", "q_next_all"),
          2: ("sel_conv1", "sel_conv2", "sel_conv3", "sel_h1", "q_sel_all")}
SHAPE = {"a1": (20, 20, 32), "a2": (9, 9, 64), "a3": (7, 7, 64), "h1": (512,)}


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


def probed(a, slot, n, A, q=None):
    """a1, a2, a3, h1 and q of one instance of the last forward (q: the rows a qvalues call returned)"""
    dev = {k: a.probe(p, n * int(np.prod(SHAPE[k]))).reshape(n, *SHAPE[k]) for k, p in zip(LAYERS, PROBES[slot])}
    dev["q"] = a.probe(PROBES[slot][4], n * A).reshape(n, A) if q is None else np.asarray(q, np.float32)
    return dev


def check_instance(params, obs, dev, split, label, only=Fw.OPS):
    """The probed layers of one instance against the reference on the probed inputs.  Prints the device's ratios; returns them."""
    inp = dict(params=params, obs=obs, **{k: dev[k] for k in LAYERS})
    for k in LAYERS:
        assert (dev[k] == 0).any() and (dev[k] > 0).any(), "a vacuous case: %s of %s" % (k, label)
    assert (dev["q"] != 0).all() and np.unique(dev["q"]).size > dev["q"].size // 2, "a vacuous case: q of %s" % label
    ops = Fw.reference(inp, split, only)
    val = {k: dev[k] for k in only}
    ratios = Fw.sharp_ratios(ops, val)
    print("forward ratios %s: " % label + " ".join("%s %.3f" % (k, ratios[k]) for k in only))
    Fw.check_all(ops, val, Fw.LAMBDA)
    if "a1" in only:   # where every product is 0 (zero pixels under every tap) conv1's epilogue leaves relu(b1) to the bit
        mask, b1 = Fw.bias_only(inp)
        assert np.array_equal(dev["a1"][mask].view(np.uint32), np.ascontiguousarray(b1[mask]).view(np.uint32)), label
    return ratios


def has_edges(Bsz, obs, nobs):
    (z0, z1), (f0, f1) = Fw.EDGE_ROWS[Bsz]
    return (obs[z0] == 0).all() and (nobs[z1] == 0).all() and (obs[f0] == 255).all() and (nobs[f1] == 255).all()


def run_case(B, Bsz, A, ns, ddqn, label, profile=False, **kw):
    q, tg, shapes = Fw.case_params(A, ns, Bsz)
    pq, pt = Fw.unflat(q, shapes), Fw.unflat(tg, shapes)
    obs, act, nobs, rew, term = Fw.case_batch(Bsz, A, ns)
    if Bsz in Fw.EDGE_ROWS:
        assert has_edges(Bsz, obs, nobs)
    split = kw.get("arithmetic", "bf16x3_6") == "bf16x3_6"
    a = make_agent(B, Bsz, A, ns, ddqn, **kw)
    try:
        a.set_params(q, "qnet"); a.set_params(tg, "qnet_tgt")
        if profile:
            a.profile_enable(True)
        a.update_on_batch(obs, act, nobs, rew, term)      # lr 1e-4: the parameters move, the probed buffers are the forward's
        if profile:   # one launch per layer, all instances in each: the labels tell this form from the fused one, which has none
            names = list(a.profile_read())
            for k in ("fwd_conv1", "fwd_conv2", "fwd_conv3", "fwd_l1", "head_fwd_td"):
                assert k in names, (k, names)
            a.profile_enable(False)
        check_instance(pq, obs, probed(a, 0, Bsz, A), split, label + " slot 0")
        check_instance(pt, nobs, probed(a, 1, Bsz, A), split, label + " slot 1")
        if ddqn:
            check_instance(pq, nobs, probed(a, 2, Bsz, A), split, label + " slot 2")
        else:
            with pytest.raises(B.BdrError, match="double DQN"):
                a.probe("sel_conv1", 32)
    finally:
        a.close()


def clean_env(monkeypatch, sched=None):
    for k in ("BDR_SCHED", "BDR_DQN_F32_EXACT"):
        monkeypatch.delenv(k, raising=False)
    if sched is not None:
        monkeypatch.setenv("BDR_SCHED", sched)


IDS = ["B%d-A%d-ns%d%s" % (b, a, ns, "-ddqn" if d else "") for b, a, ns, d in Fw.CASES]
MID = [c for c in Fw.CASES if c[0] in (40, 65)]


@pytest.mark.parametrize("Bsz,A,ns,ddqn", Fw.CASES, ids=IDS)
def test_forward_kernels_layer_by_layer(B, monkeypatch, Bsz, A, ns, ddqn):
    clean_env(monkeypatch)
    run_case(B, Bsz, A, ns, ddqn, "B=%d A=%d ns=%d" % (Bsz, A, ns))


@pytest.mark.parametrize("Bsz,A,ns,ddqn", MID, ids=["B40", "B65-ddqn"])
def test_forward_kernels_layer_by_layer_on_one_queue(B, monkeypatch, Bsz, A, ns, ddqn):
    """BDR_SCHED=0: every instance of the update in one fused conv2+conv3 launch, both parameter sets' planes"""
    clean_env(monkeypatch, "0")
    run_case(B, Bsz, A, ns, ddqn, "B=%d A=%d ns=%d BDR_SCHED=0" % (Bsz, A, ns))


@pytest.mark.parametrize("Bsz,A,ns,ddqn", MID, ids=["B40", "B65-ddqn"])
def test_forward_kernels_layer_by_layer_in_two_launches(B, monkeypatch, Bsz, A, ns, ddqn):
    """the per-kernel profile keeps FwdC2B3 and FwdC3B3 as launches of their own: at B = 40 the last 128-row tile of both is ragged"""
    clean_env(monkeypatch)
    run_case(B, Bsz, A, ns, ddqn, "B=%d A=%d ns=%d two launches" % (Bsz, A, ns), profile=True)


@pytest.mark.parametrize("Bsz,A,ns,ddqn", MID, ids=["B40", "B65-ddqn"])
def test_forward_kernels_layer_by_layer_with_exact_arithmetic(B, monkeypatch, Bsz, A, ns, ddqn):
    clean_env(monkeypatch)
    run_case(B, Bsz, A, ns, ddqn, "B=%d A=%d ns=%d f32_exact" % (Bsz, A, ns), arithmetic="f32_exact")


def test_forward_of_opt_steps_with_the_target_on_the_other_queue(B, monkeypatch):
    """Agent::opt over a replay ring: qnet_tgt(next_obs) runs on the other queue in front of the online forward (the split forward), in the
    two-launch form, and the head kernel picks its Q rows up behind a flag.  After the first step both instances are checked (the online
    parameters are still those set); after two more, slot 1 again - the target set does not move (soft_update_interval 10000) - on the
    third batch, which the oracle ring reproduces."""
    from oracle import oracle as O
    from tests import synth
    clean_env(monkeypatch)
    cap, Bsz, A = 256, 40, 6
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=42), (4, 1, 84, 84), np.uint8)
    rb.fill_synthetic(cap, seed=3, kind=0, n_actions=A)
    rows = synth.atari_rows(3, 0, cap)
    oref = O.Replay(cap, 42, 28224, 8)
    oref.push(rows[0], rows[1].reshape(-1, 1), rows[2], rows[3], rows[4], rows[5])
    q, tg, shapes = Fw.case_params(A, 4, Bsz)
    pq, pt = Fw.unflat(q, shapes), Fw.unflat(tg, shapes)
    a = make_agent(B, Bsz, A, 4, False)
    try:
        a.set_params(q, "qnet"); a.set_params(tg, "qnet_tgt")
        a.opt(rb)
        b = oref.batch(Bsz)
        obs, nobs = b["obs"].reshape(Bsz, 4, 84, 84), b["next_obs"].reshape(Bsz, 4, 84, 84)
        check_instance(pq, obs, probed(a, 0, Bsz, A), True, "opt x 1, B=40 slot 0")
        check_instance(pt, nobs, probed(a, 1, Bsz, A), True, "opt x 1, B=40 slot 1")
        for _ in range(2):
            a.opt(rb)
            b = oref.batch(Bsz)
        assert np.array_equal(a.get_params("qnet_tgt"), tg) and not np.array_equal(a.get_params("qnet"), q)
        check_instance(pt, b["next_obs"].reshape(Bsz, 4, 84, 84), probed(a, 1, Bsz, A), True, "opt x 3, B=40 slot 1")
    finally:
        a.close(); rb.close()


@pytest.mark.parametrize("ns", range(1, 9))
def test_conv1_of_every_n_stack_in_both_forms(B, monkeypatch, ns):
    """k_conv1_bf16<NS> (n_stack 7, 8) and k_conv1_bf16_img<NS, 1, 512> from an update at B = 2, then the acting call's
    k_conv1_bf16_img<NS, 1, 1024> (n_stack <= 6; above, the direct form again) on the same images: each against the reference, and the
    two a1 the same words - the bit identity the kernels' headers promise."""
    clean_env(monkeypatch)
    Bsz, A = 2, 6
    q, tg, shapes = Fw.case_params(A, ns, Bsz)
    pq = Fw.unflat(q, shapes)
    rng = np.random.default_rng(700 + ns)
    obs, nobs = (rng.integers(0, 256, (Bsz, ns, 84, 84), dtype=np.uint8) for _ in range(2))
    obs[1, :, :40] = 0                       # positions with no product at all, positions with a few
    act, rew, term = np.array([1, 2], np.int64), np.array([0.5, -0.25], np.float32), np.zeros(Bsz, np.int8)
    a = make_agent(B, Bsz, A, ns, False)
    try:
        a.set_params(q, "qnet"); a.set_params(tg, "qnet_tgt")
        a.update_on_batch(obs.reshape(Bsz, ns, 1, 84, 84), act, nobs.reshape(Bsz, ns, 1, 84, 84), rew, term)
        trained = probed(a, 0, Bsz, A)
        check_instance(pq, obs, trained, True, "conv1 ns=%d update" % ns, only=("a1",))
        a.set_params(q, "qnet")              # the update stepped the online set
        rows = a.qvalues(obs.reshape(Bsz, ns, 1, 84, 84))
        acting = probed(a, 0, Bsz, A, q=rows)
        check_instance(pq, obs, acting, False, "conv1 ns=%d acting" % ns)
        assert np.array_equal(trained["a1"].view(np.uint32), acting["a1"].view(np.uint32))
    finally:
        a.close()


def test_acting_forward_layer_by_layer(B, monkeypatch):
    """qvalues on n rows: n <= 8 the acting kernels (conv1 with 16 waves, k_act_layer<2>, <3> and <0>: f32 fmaf chains, partials handed
    across XCDs through a last-workgroup ticket, l2 in the last workgroup; n = 8 twice in a row: the tickets re-arm), above that the
    training kernels with one instance and no TD step (split arithmetic)."""
    clean_env(monkeypatch)
    A, ns = 6, 4
    q, tg, shapes = Fw.case_params(A, ns, 24)
    pq = Fw.unflat(q, shapes)
    obs = np.random.default_rng(77).integers(0, 256, (24, ns, 84, 84), dtype=np.uint8)
    obs[3] = 0; obs[4] = 255
    a = make_agent(B, 32, A, ns, False)
    try:
        a.set_params(q, "qnet"); a.set_params(tg, "qnet_tgt")
        first8 = None
        for n in (1, 5, 8, 8, 9, 24):
            rows = a.qvalues(obs[:n].reshape(n, ns, 1, 84, 84))
            assert rows.shape == (n, A)
            dev = probed(a, 0, n, A, q=rows)
            assert np.array_equal(a.probe("q_pred_all", n * A).reshape(n, A).view(np.uint32), rows.view(np.uint32))   # the returned rows are the device's
            check_instance(pq, obs[:n], dev, n > 8, "acting n=%d" % n)
            if n == 8:
                if first8 is not None:
                    assert all(np.array_equal(first8[k].view(np.uint32), dev[k].view(np.uint32)) for k in Fw.OPS)
                first8 = dev
    finally:
        a.close()
