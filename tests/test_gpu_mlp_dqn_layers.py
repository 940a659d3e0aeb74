"""Every kernel of the Mlp DQN step against the f64 reference of its own layer (tests/mlp_dqn_layer_reference.py), on the device's own
inputs.

One or more `update_on_batch` calls per case; every raw buffer of the update is read back with `Dqn.layer` and every GEMM output goes
through `check`: (a) S == 0 -> exactly 0 (all padding, masked units, an empty row chunk), (b) |err| <= n u S, (c) |err| <= lambda
sqrt(n) u S.  The pack, the TD rows, the loss mean and the one-hot gradient row are held to the bits of their f32 restatement, the
optimizer to optimizer_inputs.adam_f32 of the read-back gradient.  Each case prints one "mlp dqn layer ratios" line (largest |err| /
(sqrt(n) u S) per output, chunks folded: compare it with the table below).

  case (in, units, actions, batch)                      what it reaches
  c1-double     4 (64,64) 2 B=32 double SmoothL1 tie    three instances; every wave's first block prefetched; the selector ties on every row
  two-blocks    4 (64,64) 2 B=64 all-terminal           two full row blocks; the LDS plan (156 672 B) does not fit: one-workgroup global by default
  ragged-lds    4 (64,64) 2 B=48 SmoothL1 weighted clip second row block of 16 rows, resident in LDS; all three clip states
  ragged-deep   7 (64,64,64) 5 B=33                     four layers; a row block of one row
  one-row       3 (64,) 3 B=1
  wide-in       100 (64,) 33 B=17                       Kp = 128: mf_block's long-K loop beside prefetched blocks; > 32 actions in the 16-lane argmax
  wide-hidden   5 (128,) 6 B=32 activation_out          12 backward blocks for 8 waves; rows clamped to 0
  a64-double    4 (64,) 64 B=32 double                  all 64 action columns real
  (each of the above by default and with BDR_NO_MLP_LDS=1)
  l-65          4 (64,64) 2 B=65 plain tie / double SmoothL1 tie    row-block head; third row block of one row
  l-wide-head   6 (64,192) 5 B=33 activation_out        k_td_dense + k_mean_rows; -fused: BDR_MLP_HEAD_FUSE_WIDE=1, the head with three column groups
  l-a33         9 (96,) 33 B=40 weighted clip           no head; k_td_dense with lanes 32..63 live
  l-a64-double  4 (64,) 64 B=33 double SmoothL1
  l-chunks      11 (64,64) 3 B=515, 4100, 40            2 chunks; 16 chunks of 288 rows, chunk 15 empty; 40 rows fit the one-workgroup step
  l-chunks-layers  the same with BDR_NO_MLP_FUSED=1     40 rows: planned 16 chunks, launched 1 - stale partials must not enter
  l-deep        3 (64,128,64,96,64,64,32,64) 4 B=33     nine layers
  l-wide-k      5 (512,64) 2 B=33                       two passes of dense_small_tile's kb loop
  l-big-tiles   4 (128,96) 3 B=130 BDR_NO_SMALL_GEMM=1  k_igemm, k_igemm_red<DenseDw>, launch_adam

Largest |err| / (sqrt(n) u S) per output over every case: restatement (CPU, sequential f32; RESTATEMENT_RATIO) | MI355X (a record) |
lambda.  A `.sum` is exact (0) with one chunk.
  dy0       0.986 | 0.986 | 3.94    dy1       0.995 | 0.998 | 3.98    dy2       0.987 | 0.988 | 3.95
  dy3       0.443 | 0.236 | 1.77    dy4       0.391 | 0.372 | 1.56    dy5       0.750 | 0.378 | 3.00
  dy6       0.450 | 0.212 | 1.80    dy7       0.967 | 0.967 | 3.87    gW0       1.098 | 0.991 | 4.39
  gW1       1.000 | 1.038 | 4.00    gW2       0.888 | 0.930 | 3.55    gW3       0.723 | 0.896 | 2.89
  gW0.part  1.007 | 0.885 | 4.03    gW1.part  1.000 | 1.034 | 4.00    gW2.part  0.920 | 0.784 | 3.68
  gW3.part  1.114 | 0.963 | 4.46    gW4.part  0.890 | 0.823 | 3.56    gW5.part  0.491 | 0.217 | 1.96
  gW6.part  0.261 | 0.133 | 1.04    gW7.part  0.276 | 0.172 | 1.10    gW8.part  0.747 | 0.730 | 2.99
  gW0.sum   0.698 | 0.707 | 2.79    gW1.sum   0.706 | 0.707 | 2.82    gW2.sum   0.643 | 0.704 | 2.57
  gW3.sum   0.000 | 0.000 | 1.00    gW4.sum   0.000 | 0.000 | 1.00    gW5.sum   0.000 | 0.000 | 1.00
  gW6.sum   0.000 | 0.000 | 1.00    gW7.sum   0.000 | 0.000 | 1.00    gW8.sum   0.000 | 0.000 | 1.00
  z0.h0     1.122 | 1.070 | 4.49    z0.h1     0.587 | 0.380 | 2.35    z0.h2     0.356 | 0.300 | 1.42
  z0.h3     0.346 | 0.192 | 1.38    z0.h4     0.172 | 0.121 | 1.00    z0.h5     0.191 | 0.092 | 1.00
  z0.h6     0.117 | 0.109 | 1.00    z0.h7     0.316 | 0.240 | 1.26    z0.h8     0.145 | 0.118 | 1.00
  z1.h0     1.113 | 1.113 | 4.45    z1.h1     0.479 | 0.374 | 1.92    z1.h2     0.380 | 0.432 | 1.52
  z1.h3     0.192 | 0.199 | 1.00    z1.h4     0.128 | 0.126 | 1.00    z1.h5     0.156 | 0.141 | 1.00
  z1.h6     0.172 | 0.108 | 1.00    z1.h7     0.315 | 0.187 | 1.26    z1.h8     0.125 | 0.077 | 1.00
  z2.h0     0.939 | 0.939 | 3.76    z2.h1     0.363 | 0.353 | 1.45    z2.h2     0.117 | 0.098 | 1.00
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_dqn_layer_reference as X  # noqa: E402

ENV_KEYS = ("BDR_NO_STEP_GATHER", "BDR_NO_MLP_LDS", "BDR_NO_MLP_FUSED", "BDR_NO_MLP_HEAD_FUSE", "BDR_MLP_HEAD_FUSE_WIDE", "BDR_NO_SMALL_GEMM", "BDR_STEP_GRAPH")
NO_LDS = (("BDR_NO_MLP_LDS", "1"),)
NO_HEAD = (("BDR_NO_MLP_HEAD_FUSE", "1"),)
RUNS = [(c.name, env) for c in X.CASES.values() for env in (((), NO_LDS) if c.one_wg else ((),))]
ARENAS = ("q", "q_tgt", "grad", "m", "v")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def make_agent(B, c: X.Case, mp, env=()):
    """the switches are read at creation: cleared and set before Dqn.build"""
    for k in ENV_KEYS: mp.delenv(k, raising=False)
    for k, v in tuple(c.env) + tuple(env): mp.setenv(k, v)
    cfg = B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.MlpConfig(in_dim=c.in_dim, units=tuple(c.units), out_dim=c.A, activation_out=c.act_out),
                                                    opt_config=B.OptimizerConfig.Adam(X.LR)),
                      batch_size=c.capacity, discount_factor=X.GAMMA, double_dqn=c.double, critic_loss=c.loss, soft_update_interval=10000,
                      clip_td_err=tuple(c.clip) if c.weighted else None, device=0)
    a = B.Dqn.build(cfg)
    q, qt = X.case_params(c)
    a.set_params(q, "qnet"); a.set_params(qt, "qnet_tgt")   # different values: an instance mix-up shows
    return a


def probed_update(a, c: X.Case, step: int, before=None) -> dict:
    """One update_on_batch -> the `inp` of X.reference / X.exact from the device's own buffers.  before: the previous update's inp."""
    Bn, L = c.batches[step], c.L
    if before is None:   # (the probe serves nothing before the first update: the arenas as set, zero moments)
        q0, qt0 = X.to_arena(a.get_params("qnet"), c), X.to_arena(a.get_params("qnet_tgt"), c)
        m0, v0 = np.zeros_like(q0), np.zeros_like(q0)
    else:
        q0, qt0, m0, v0 = before["q1"], before["qt1"], before["m1"], before["v1"]
    obs, act, nobs, rew, term, w = X.case_batch(c, Bn, step)
    a.update_on_batch(obs, act, nobs, rew, term, weight=w)
    g = lambda buf, z=0, l=0: a.layer(buf, Bn, z, l)
    form = a.step_form
    chunks = g("chunks") if form.startswith("layers") else 0
    inp = dict(case=c, B=Bn, form=form, chunks=chunks, t=step + 1, obs=obs, nobs=nobs, act=act, reward=rew, term=term, weight=w,
               q0=q0, qt0=qt0, m0=m0, v0=v0, x_in=[g("x_in", z) for z in range(c.nz)], acts=[[g("act", z, l) for l in range(L)] for z in range(c.nz)],
               dy=[g("dy", 0, l) for l in range(L)], pred=g("pred"), tgt=g("tgt"), loss_row=g("loss_row"), td_abs=g("td_abs"), loss=g("loss"),
               part=[g("dw_part", 0, l) for l in range(L)] if chunks else None, grad=g("grad"), q1=g("q"), qt1=g("q_tgt"), m1=g("m"), v1=g("v"))
    return inp


_runs = {}


def run_case(B, mp, name, env=()):
    """every update of a case on one agent, probed; run once per (case, switches) and shared"""
    key = (name, tuple(env))
    if key not in _runs:
        c = X.CASES[name]
        a = make_agent(B, c, mp, env)
        out, inp = [], None
        for step in range(len(c.batches)):
            inp = probed_update(a, c, step, inp)
            out.append(inp)
        a.close()
        _runs[key] = out
    return _runs[key]


@pytest.mark.parametrize("name,env", RUNS, ids=["%s%s" % (n, "-global" if e else "") for n, e in RUNS])
def test_every_kernel_against_its_layer(B, name, env, monkeypatch):
    c = X.CASES[name]
    bad = []
    for step, inp in enumerate(run_case(B, monkeypatch, name, env)):
        Bn = c.batches[step]
        ops, dev = X.reference(inp), X.device(inp)
        r = X.ratios(ops, dev)
        print("mlp dqn layer ratios %s%s B=%d %s chunks=%d: %s" % (name, "-global" if env else "", Bn, inp["form"], inp["chunks"],
                                                                      " ".join("%s %.3f" % kv for kv in sorted(r.items()))))
        want = X.predict_form(c, Bn, env)
        if inp["form"] != want: bad.append("B=%d: the step took form %s, predicted %s" % (Bn, inp["form"], want))
        if inp["chunks"] != X.predict_chunks(c, Bn, want): bad.append("B=%d: %d chunks, predicted %d" % (Bn, inp["chunks"], X.predict_chunks(c, Bn, want)))
        bad += ["B=%d: %s" % (Bn, m) for m in X.failures(ops, X.exact(inp), dev) + X.padding_failures(inp)]
    assert not bad, "\n".join(bad)


def same_bits(x, y, what):
    bad = []
    for k in ("x_in", "acts", "dy", "pred", "tgt", "loss_row", "td_abs", "loss", "grad", "q1", "qt1", "m1", "v1"):
        flat = lambda v: [v] if isinstance(v, np.ndarray) else [e for s in v for e in flat(s)]
        for i, (p, q) in enumerate(zip(flat(x[k]), flat(y[k]))):
            if not np.array_equal(X.bits(p), X.bits(q)): bad.append("%s: %s[%d] differs in %d elements" % (what, k, i, (X.bits(p) != X.bits(q)).sum()))
    return bad


@pytest.mark.parametrize("name", [c.name for c in X.CASES.values() if c.one_wg])
def test_lds_and_global_forms_leave_the_same_bits(B, name, monkeypatch):
    """every probed buffer and arena, not the parameters alone"""
    lds, glb = run_case(B, monkeypatch, name), run_case(B, monkeypatch, name, NO_LDS)
    assert glb[0]["form"] == "global" and lds[0]["form"] == X.predict_form(X.CASES[name], X.CASES[name].batches[0])
    bad = same_bits(lds[0], glb[0], name)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["l-65", "l-65-double", "l-wide-head"])
def test_head_fused_and_unfused_give_the_same_bits(B, name, monkeypatch):
    if name == "l-wide-head":
        fused, unfused = run_case(B, monkeypatch, "l-wide-head-fused"), run_case(B, monkeypatch, "l-wide-head")
    else:
        fused, unfused = run_case(B, monkeypatch, name), run_case(B, monkeypatch, name, NO_HEAD)
    assert fused[0]["form"] == "layers_head" and unfused[0]["form"] == "layers_td"
    bad = same_bits(fused[0], unfused[0], name)
    for l in range(X.CASES[name].L):
        if not np.array_equal(X.bits(fused[0]["part"][l]), X.bits(unfused[0]["part"][l])): bad.append("partials of layer %d differ" % l)
    assert not bad, "\n".join(bad)


def test_the_probe_refuses_and_changes_nothing(B, monkeypatch):
    from border_amd import _lib
    INVALID = 1
    c = X.CASES["l-65-double"]
    a, quiet = make_agent(B, c, monkeypatch), make_agent(B, c, monkeypatch)
    out = np.full(1 << 16, 7.0, np.float32)
    call = lambda h, buf, z, l, n: _lib.lib().bdr_dqn_mlp_layer_probe(h, buf, z, l, out.ctypes.data_as(C.c_void_p), n)
    tot, Bn = X.total(c), 65
    for buf, n in ((a.BUFS["q"], tot), (a.BUFS["pred"], Bn), (a.BUFS["form"], 1), (a.BUFS["chunks"], 1)):
        assert call(a.handle, buf, 0, 0, n) == INVALID, "served before any update"
    for step in range(3):
        batch = X.case_batch(c, Bn, step)
        a.update_on_batch(*batch[:5]); quiet.update_on_batch(*batch[:5])
        if step < 2:
            for z in range(c.nz):
                a.layer("x_in", Bn, z)
                for l in range(c.L): a.layer("act", Bn, z, l)
            for l in range(c.L): a.layer("dy", Bn, 0, l); a.layer("dw_part", Bn, 0, l)
            for k in ("pred", "tgt", "loss_row", "td_abs", "loss") + ARENAS: a.layer(k, Bn)
    for k in ARENAS:
        assert np.array_equal(X.bits(a.layer(k, Bn)), X.bits(quiet.layer(k, Bn))), "probing changed " + k
    bufs = a.BUFS
    refused = [("a wrong float count", bufs["pred"], 0, 0, Bn + 1), ("a short float count", bufs["act"], 0, 0, Bn * 64 - 1), ("rows of another batch", bufs["x_in"], 0, 0, 64 * 64),
               ("an arena one float short", bufs["grad"], 0, 0, tot - 1), ("z >= nz", bufs["act"], 3, 0, Bn * 64), ("z < 0", bufs["x_in"], -1, 0, Bn * 64),
               ("a layer out of range", bufs["act"], 0, c.L, Bn * 64), ("a negative layer", bufs["dy"], 0, -1, Bn * 64),
               ("an instance on dy", bufs["dy"], 1, 0, Bn * 64), ("a layer on x_in", bufs["x_in"], 0, 1, Bn * 64), ("an index on pred", bufs["pred"], 0, 1, Bn),
               ("an index on an arena", bufs["q"], 1, 0, tot), ("an index on form", bufs["form"], 0, 1, 1), ("an index on chunks", bufs["chunks"], 1, 0, 1),
               ("an unknown buffer", 16, 0, 0, 1), ("a negative buffer", -1, 0, 0, 1)]
    for what, buf, z, l, n in refused:
        assert call(a.handle, buf, z, l, n) == INVALID, what + " was served"
    assert (out == 7.0).all(), "a refused call wrote to the output"
    plain = make_agent(B, X.CASES["l-65"], monkeypatch)      # two instances: z = 2 has no rows
    plain.update_on_batch(*X.case_batch(X.CASES["l-65"], 65)[:5])
    assert call(plain.handle, bufs["act"], 2, 0, 65 * 64) == INVALID and call(plain.handle, bufs["x_in"], 2, 0, 65 * 64) == INVALID
    one = make_agent(B, X.CASES["c1-double"], monkeypatch)   # a one-workgroup step forms no partials
    one.update_on_batch(*X.case_batch(X.CASES["c1-double"], 32)[:5])
    assert one.step_form == "lds"
    assert call(one.handle, bufs["dw_part"], 0, 0, 64 * 64 + 64) == INVALID and call(one.handle, bufs["chunks"], 0, 0, 1) == INVALID
    sac = B.Sac.build(B.SacConfig(obs_dim=3, act_dim=1, pi_units=(64,), q_units=(64,), batch_size=4, device=0))
    assert call(sac.handle, bufs["form"], 0, 0, 1) == INVALID, "a SAC handle was served"
    assert (out == 7.0).all()
    for x in (a, quiet, plain, one, sac): x.close()


def test_a_layer_form_group_member_equals_its_twin_in_every_buffer(B, monkeypatch):
    from tests.test_gpu_agent_group import Ring, cfg
    for k in ENV_KEYS: monkeypatch.delenv(k, raising=False)
    members = [(cfg(B, 4, (64, 64), 2, 65, double_dqn=True, critic_loss="SmoothL1", param_seed=21), 31), (cfg(B, 4, (64, 64), 2, 65, double_dqn=True, param_seed=22), 32)]
    c = X.Case("group", 4, (64, 64), 2, (65,), double=True)

    def read(a):
        g = lambda buf, z=0, l=0: a.layer(buf, 65, z, l)
        d = dict(form=a.step_form, chunks=g("chunks"), x_in=[g("x_in", z) for z in range(3)], acts=[[g("act", z, l) for l in range(3)] for z in range(3)],
                 dy=[g("dy", 0, l) for l in range(3)], part=[g("dw_part", 0, l) for l in range(3)], grad=g("grad"), q1=g("q"), qt1=g("q_tgt"), m1=g("m"), v1=g("v"))
        for k in ("pred", "tgt", "loss_row", "td_abs", "loss"): d[k] = g(k)
        return d
    grp = B.DqnGroup.build([m for m, _ in members])
    assert grp.form == "layers"
    rings = [Ring(B, m, seed) for m, seed in members]
    for r in rings: r.push(40)
    grp.opt([r.rb for r in rings]); grp.sync()
    got = [read(m) for m in grp.members]
    grp.close()
    for r in rings: r.rb.close()
    bad = []
    for i, (m, seed) in enumerate(members):
        a, ring = B.Dqn.build(m), Ring(B, m, seed)
        ring.push(40)
        a.opt(ring.rb); a.sync()
        want = read(a)
        a.close(); ring.rb.close()
        assert got[i]["form"] == want["form"] == "layers_head" and got[i]["chunks"] == want["chunks"] == 1
        bad += same_bits(got[i], want, "member %d" % i)
        for l in range(c.L):
            if not np.array_equal(X.bits(got[i]["part"][l]), X.bits(want["part"][l])): bad.append("member %d: partials of layer %d differ" % (i, l))
    assert not bad, "\n".join(bad)
