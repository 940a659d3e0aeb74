"""Every kernel of the SAC step against the f64 reference of its own layer (tests/sac_layer_reference.py), on the device's own inputs.

One or more `update_on_batch` calls per case with `Sac.keep_layers(True)`; every raw buffer is read back with `Sac.layer` in both
phases and every output goes through `check`: (a) S == 0 -> exactly 0 (all padding, masked units, the unselected critic's gradient),
(b) |err| <= n u S, (c) |err| <= lambda sqrt(n) u S.  No element is exempt, saturated rows included.  Each case prints one
"sac layer ratios" line (largest |err| / (sqrt(n) u S) per output, critics and chunks folded: compare it with the table below) and the
device's function errors.

  case           shape                                                      what it reaches
  tiny-padded    B=3 O=5 A=2 pi(64) q(64) NC=1 Fix Mse                      a row block almost all padding; n_trunk 1; two-layer critic (tail_here)
  a17-edge       B=33 O=15 A=17 pi(96,40) q(72,136) NC=2 Auto SmoothL1 rs   sac_heads_row in k_sac_heads_action; (O%32)+A == 32; a row block of one row
  a32            B=40 O=32 A=32 pi(64) q(64,64)                             n0a == col0; full-width heads
  unfused-a33    B=65 O=9 A=33; unfused-o30: O=30 A=8                        k_sac_action, k_sac_select, k_sac_actor_grad, k_sac_critic_td, dense_dx with accum
  chain          B=72 O=17 A=6 pi(256,256) q(256,256)                       BDR_SAC_CHAIN_TPW unset / 1 / 4, BDR_SAC_HEADS_FUSE=1
  chain-ragged   pi(256,40) q(256,136) NC=3                                 n1 = 64 / 192; 4 + 2 passes
  wide-k         B=33 q(512,64)                                             two passes of dense_small_tile's kb loop
  chunked-dw     O=11 A=3 pi(64) q(64,64) NC=3, B = 515, 1290, 40 in turn    2 chunks (last wave 8 rows); 5 chunks (c + q < chunks); planned 5, launched 1
  deep           B=33 pi(128,64,32) q(64,64,64,64) NC=4                     20 dW jobs in two grouped launches; the pi_dx loop
  big-tiles      B=130 BDR_NO_SMALL_GEMM=1                                  k_igemm; k_igemm_red_group with 2 chunks
  saturated      B=64 O=8 A=4, heads x 14, two bit-identical critics        a == +-1.0f, all three clamp states, every row a tie -> critic 0
  logf-probe     B=64 O=3 A=1                                               log p is one log term: the device's logf error

Largest |err| / (sqrt(n) u S) per output (critics and chunks folded: the keys of the printed line), over every case and the acting calls:
restatement (CPU, sequential f32; tests/sac_layer_reference.py RESTATEMENT_RATIO) | MI355X (a record) | lambda.  Row-wise outputs carry
their whole bound in S (lambda 1); a `.sum` is exact (0) with one chunk; q.a.dy of the last layer is the selection one-hot.
  loss_actor   0.079 | 0.129 | 1.00    loss_critic  0.100 | 0.100 | 1.00    lrow         0.193 | 0.385 | 1.00
  pi'.a        0.229 | 0.260 | 1.00    pi'.e        0.306 | 0.223 | 1.22    pi'.h0       1.129 | 0.987 | 4.52
  pi'.h1       0.464 | 0.317 | 1.86    pi'.h2       0.183 | 0.121 | 1.00    pi'.logp     0.114 | 0.341 | 1.00
  pi'.mean     0.434 | 0.271 | 1.74    pi.a         0.540 | 0.383 | 1.00    pi.dW0.part  1.051 | 0.920 | 4.20
  pi.dW0.sum   0.707 | 0.899 | 2.83    pi.dW1.part  1.063 | 1.201 | 4.25    pi.dW1.sum   0.706 | 0.707 | 2.82
  pi.dW2.part  0.860 | 0.595 | 3.44    pi.dW2.sum   0.705 | 0.705 | 2.82    pi.dW3.part  0.964 | 0.610 | 3.86
  pi.dW3.sum   0.707 | 0.696 | 2.83    pi.dW4.part  0.909 | 0.479 | 3.64    pi.dW4.sum   0.000 | 0.000 | 1.00
  pi.dy0       1.010 | 0.942 | 4.04    pi.dy1       0.685 | 0.604 | 2.74    pi.dy2       0.312 | 0.334 | 1.25
  pi.e         0.303 | 0.280 | 1.21    pi.ge        0.454 | 0.562 | 1.00    pi.gmean     0.099 | 0.240 | 1.00
  pi.h0        0.957 | 1.007 | 3.83    pi.h1        0.364 | 0.397 | 1.46    pi.h2        0.150 | 0.111 | 1.00
  pi.logp      0.099 | 0.271 | 1.00    pi.mean      0.357 | 0.279 | 1.43    pi.s         0.332 | 0.448 | 1.00
  pi.sd        0.319 | 0.402 | 1.00    q.a.dxq      0.662 | 0.571 | 2.65    q.a.dy0      0.514 | 0.514 | 2.06
  q.a.dy1      0.424 | 0.252 | 1.70    q.a.dy2      0.426 | 0.199 | 1.70    q.a.dy3      0.000 | 0.000 | 1.00
  q.a.dy4      0.000 | 0.000 | 1.00    q.a.h0       0.972 | 0.972 | 3.89    q.a.h1       0.446 | 0.317 | 1.78
  q.a.h2       0.328 | 0.269 | 1.31    q.a.h3       0.256 | 0.149 | 1.02    q.a.h4       0.145 | 0.078 | 1.00
  q.c.dy0      0.978 | 0.994 | 3.91    q.c.dy1      0.996 | 0.996 | 3.98    q.c.dy2      0.857 | 0.851 | 3.43
  q.c.dy3      0.986 | 0.983 | 3.94    q.c.dy4      0.829 | 0.829 | 3.32    q.c.h0       1.051 | 0.980 | 4.20
  q.c.h1       0.448 | 0.404 | 1.79    q.c.h2       0.368 | 0.357 | 1.47    q.c.h3       0.260 | 0.145 | 1.04
  q.c.h4       0.115 | 0.092 | 1.00    q.dW0.part   0.946 | 0.935 | 3.78    q.dW0.sum    0.707 | 0.928 | 2.83
  q.dW1.part   1.409 | 1.070 | 5.64    q.dW1.sum    0.707 | 1.020 | 2.83    q.dW2.part   1.469 | 1.121 | 5.88
  q.dW2.sum    0.704 | 0.840 | 2.82    q.dW3.part   0.996 | 1.132 | 3.98    q.dW3.sum    0.000 | 0.000 | 1.00
  q.dW4.part   0.613 | 0.406 | 2.45    q.dW4.sum    0.000 | 0.000 | 1.00    q.t.h0       0.883 | 1.046 | 3.53
  q.t.h1       0.443 | 0.326 | 1.77    q.t.h2       0.317 | 0.248 | 1.27    q.t.h3       0.249 | 0.204 | 1.00
  q.t.h4       0.154 | 0.093 | 1.00    tgt          0.371 | 0.479 | 1.00
Function errors on the MI355X against f64 libm of the same f32 argument (bar = twice the figure, rounded up): expf 1.35 u (3), tanhf 2.09 u (5),
logf 2.29 u (5).  The EntCoef Adam element is held to the bar of tests/test_gpu_optimizer_edges.py (optimizer_inputs.adam_bars).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimizer_inputs as OI  # noqa: E402
import sac_layer_reference as X  # noqa: E402

ENV_KEYS = ("BDR_NO_SMALL_GEMM", "BDR_NO_SAC_FUSE", "BDR_NO_SAC_CHAIN", "BDR_SAC_CHAIN_TPW", "BDR_SAC_HEADS_FUSE", "BDR_SAC_TAIL_IN_KERNEL",
            "BDR_STEP_GRAPH")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def make_agent(B, c: X.Case, mp, batch_size=None):
    for k in ENV_KEYS: mp.delenv(k, raising=False)
    for k, v in c.env: mp.setenv(k, v)
    cfg = B.SacConfig(obs_dim=c.O, act_dim=c.A, pi_units=tuple(c.pi), q_units=tuple(c.q), lr_actor=1e-3, lr_critic=2e-3, ent_coef_mode=c.ent,
                      critic_loss=c.loss, reward_scale=c.reward_scale, n_critics=c.NC, batch_size=batch_size or (c.batches or (c.B,))[0],
                      gamma=c.gamma, epsilon=c.eps, min_lstd=c.lo, max_lstd=c.hi, device=0)
    a = B.Sac.build(cfg)
    pi, qs = X.case_params(c)
    a.set_params(pi, "pi")
    for i in range(c.NC):
        a.set_params(qs[i], f"qnet_{i}"); a.set_params(qs[i], f"qnet_tgt_{i}")
    return a


def probed_update(a, c: X.Case, Bn: int, step: int) -> dict:
    """One update_on_batch with the snapshot on -> the `inp` of X.reference from the device's own buffers."""
    nt, L, NC = len(c.pi), len(c.q) + 1, c.NC
    pi0 = a.get_params("pi")
    q0 = [a.get_params(f"qnet_{i}") for i in range(NC)]
    qt0 = [a.get_params(f"qnet_tgt_{i}") for i in range(NC)]
    la0 = a.get_params("log_alpha")
    la_before = {k: a.get_params("log_alpha", r) for k, r in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq"))}
    batch = X.case_batch(c, Bn, step)
    a.keep_layers(True)
    a.update_on_batch(*batch)
    pi1 = a.get_params("pi")
    inp = dict(case=c, B=Bn, pi0=X.internal(pi0, c, "pi"), pi1=X.internal(pi1, c, "pi"), q=[X.internal(x, c, "q") for x in q0],
               qt=[X.internal(x, c, "q") for x in qt0], reward=batch[3], term=batch[4], log_alpha0=la0)
    g = lambda buf, ph, i=0, l=0: a.layer(buf, Bn, ph, i, l)
    Aph = {k: g(k, "actor") for k in ("x_o", "z", "mean", "e", "a_s", "s_s", "sd_s", "logp", "xq_a", "gmean", "ge", "log_alpha")}
    Aph["t_act"] = [g("t_act", "actor", 0, l) for l in range(nt)]
    Aph["t_dy"] = [g("t_dy", "actor", 0, l) for l in range(nt)]
    for k in ("c_act", "c2_act", "c_dy"):
        Aph[k] = [[g(k, "actor", i, l) for l in range(L)] for i in range(NC)]
    if not c.fused:   # (the row-block kernels never form it: refused there)
        Aph["dxq"] = [g("dxq", "actor", i) for i in range(NC)]
    Cph = {k: g(k, "critic") for k in ("x_no", "z", "mean", "e", "logp", "xq_n", "xq_c", "tgt", "log_alpha", "lrow", "scal", "pi_grad")}
    Cph["t_act"] = [g("t_act", "critic", 0, l) for l in range(nt)]
    for k in ("c_act", "c2_act", "c_dy"):
        Cph[k] = [[g(k, "critic", i, l) for l in range(L)] for i in range(NC)]
    inp["pi_chunks"] = [a.layer("pi_chunks", Bn, "critic", 0, l) for l in range(nt + 2)]
    inp["q_chunks"] = [a.layer("q_chunks", Bn, "critic", 0, l) for l in range(L)]
    Cph["pi_part"] = [g("pi_part", "critic", 0, l) for l in range(nt + 2)]
    Cph["q_part"] = [[g("q_part", "critic", i, l) for l in range(L)] for i in range(NC)]
    Cph["q_grad"] = [g("q_grad", "critic", i) for i in range(NC)]
    Aph["xq_c"] = Cph["xq_c"]   # written by the pack launch and never again: the critic phase's buffer is the actor phase's input
    inp["actor"], inp["critic"] = Aph, Cph
    inp["la_before"] = la_before
    inp["la_after"] = {k: a.get_params("log_alpha", r) for k, r in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq"))}
    # what the critic phase does not touch is the same memory in both phases
    for i in range(NC):
        for l in range(L):
            assert np.array_equal(Aph["c2_act"][i][l], Cph["c2_act"][i][l])
    assert np.array_equal(Aph["log_alpha"], Cph["log_alpha"])
    return inp


def check_log_alpha(inp, t):
    """EntCoef::update's Adam element (step t of its own counter) against f64 under the bar of tests/test_gpu_optimizer_edges.py.  Its
    gradient -(sum(log_p + target) / B) is restated exactly: the block partials (probed on the fused path, the 32-lane butterfly of the
    probed rows otherwise) added one by one in block order, one division - all IEEE operations in a fixed order."""
    c, Bn = inp["case"], inp["B"]
    if c.ent[0] != "Auto":
        for k in "pmv": assert np.array_equal(inp["la_before"][k], inp["la_after"][k]), "a fixed entropy coefficient does not move"
        return
    if c.fused:
        part = np.asarray(inp["critic"]["lrow"][0], np.float32)
    else:
        nb = (Bn + 31) // 32
        v = np.zeros(nb * 32, np.float32)
        v[:Bn] = np.asarray(inp["actor"]["logp"], np.float32) + np.float32(c.ent[1])
        v = v.reshape(nb, 32)
        for off in (16, 8, 4, 2, 1):
            v = (v + v[:, np.arange(32) ^ off]).astype(np.float32)
        part = v[:, 0]
    tot = np.float32(0)
    for x in part: tot = np.float32(tot + x)
    g = np.asarray([-(tot / np.float32(Bn))], np.float32)
    s = OI.adam_scalars(False, c.ent[2], 0, 0, 0, 0, t)
    b, after = inp["la_before"], inp["la_after"]
    (r64, _), bars = OI.adam_f64(b["p"], g, b["m"], b["v"], None, s), OI.adam_bars(b["p"], g, b["m"], b["v"], None, s)
    for k, r in zip("pmv", r64):
        d = np.abs(np.asarray(after[k], np.float64) - r)
        assert (d <= bars[k]).all(), ("log_alpha", k, float(after[k][0]), float(r[0]), float(bars[k][0]))
    assert np.array_equal(after["p"], inp["actor"]["log_alpha"]), "the snapshot's log_alpha is the stepped one"


def check_update(inp, tag):
    c = inp["case"]
    ops, dev = X.reference(inp), X.device(inp)
    assert set(ops) == set(dev)
    fe = X.function_errors(inp)
    print("sac layer ratios %s:" % tag, " ".join("%s %.3f" % kv for kv in sorted(X.kind_ratios(ops, dev).items())), "| chunks pi", inp["pi_chunks"], "q", inp["q_chunks"])
    print("function errors %s:" % tag, " ".join(("%s %d" if k.endswith("_rows") else "%s %.2f u") % (k, v) for k, v in sorted(fe.items())))
    bad = X.branch_checks(inp) + X.exact_checks(inp) + X.failures(ops, dev)
    assert not bad, "\n".join(bad)
    for k in X.FUNC_U:
        assert fe.get(k, 0.0) <= X.FUNC_U[k], (k, fe[k], X.FUNC_U[k])
    assert "logf" in fe or c.A != 1, "too few rows on which logf's own error is observable"
    return fe


@pytest.mark.parametrize("name", list(X.CASES))
def test_sac_layers(B, monkeypatch, name):
    c = X.CASES[name]
    a = make_agent(B, c, monkeypatch)
    try:
        for step, Bn in enumerate(c.batches or (c.B,)):
            inp = probed_update(a, c, Bn, step)
            if c.special == "saturated":
                L = len(c.q) + 1
                qa = np.stack([inp["actor"]["c_act"][i][L - 1][:, 0] for i in range(c.NC)])
                assert (qa[0] == qa[1]).all(), "bit-identical critics tie on every row"
                assert (inp["actor"]["c_dy"][0][L - 1][:, 0] == 1).all() and not inp["actor"]["c_dy"][1][L - 1].any()
                assert not any(x.any() for x in inp["actor"]["c_dy"][1]), "the unselected critic's gradient is exactly 0"
                s, av = inp["actor"]["s_s"][:, :c.A], inp["actor"]["a_s"][:, :c.A]
                assert (s < c.lo).any() and ((s >= c.lo) & (s <= c.hi)).any() and (s > c.hi).any()
                assert (np.abs(av) == 1).any() and ((np.abs(av) > 0.995) & (np.abs(av) < 1)).any()
            if name == "chunked-dw":
                assert inp["q_chunks"][0] == {515: 2, 1290: 5, 40: 1}[Bn], inp["q_chunks"]
            if name == "big-tiles":
                assert inp["q_chunks"][0] == 2, inp["q_chunks"]
            check_update(inp, "%s B=%d" % (name, Bn))
            check_log_alpha(inp, step + 1)
    finally:
        a.close()


@pytest.mark.parametrize("n", [1, 8, 33])
def test_sac_acting_layers(B, monkeypatch, n):
    """Sac.sample in eval mode: the probed trunk and mean layer by layer; the action is tanhf of the probed mean (z = 0: the argument is
    the mean itself) under the tanhf bar."""
    c = X.CASES["chain"]
    a = make_agent(B, c, monkeypatch, batch_size=64)
    try:
        obs = X.case_batch(c, n, 7)[0]
        act = a.sample(obs)
        P = X.internal(a.get_params("pi"), c, "pi")
        nt, Lp = len(c.pi), X.layers(c, "pi")
        x = a.layer("x_o", n, "critic")
        assert np.array_equal(x[:, :c.O], obs) and not x[:, c.O:].any()
        ops, dev, h = {}, {}, x
        for l in range(nt):
            t = a.layer("t_act", n, "critic", 0, l)
            ops["pi.h%d" % l] = X._op("pi.h%d" % l, X.K_FWD, *X._fwd(h, P[l], Lp[l][0], True)); dev["pi.h%d" % l] = t; h = t
        mean = a.layer("mean", n, "critic")
        ops["pi.mean"] = X._op("pi.mean", X.K_HEADS, *X._fwd(h, P[nt], Lp[nt][0], False)); dev["pi.mean"] = mean
        r = np.tanh(np.asarray(mean, np.float64)[:, :c.A])
        ops["pi.a"] = X._rowwise("pi.a", "k_sac_heads_action", r, X.FUNC_U["tanhf"] * X.U * np.abs(r)); dev["pi.a"] = act
        assert np.array_equal(a.layer("a_s", n, "critic")[:, :c.A], act)
        for buf in ("tgt", "gmean", "lrow", "x_no"):   # not written by the acting call: refused until the next update
            with pytest.raises(Exception):
                a.layer(buf, n, "critic")
        print("sac layer ratios acting n=%d:" % n, " ".join("%s %.3f" % kv for kv in sorted(X.kind_ratios(ops, dev).items())))
        bad = X.failures(ops, dev)
        assert not bad, "\n".join(bad)
    finally:
        a.close()


def test_keep_layers_changes_nothing(B, monkeypatch):
    """Three updates with the snapshot on and off: parameters, moments, gradients, targets, log_alpha and probes 0..7 bit for bit."""
    c = X.CASES["a17-edge"]
    outs = []
    for on in (False, True):
        a = make_agent(B, c, monkeypatch)
        a.keep_layers(on)
        recs = [a.update_on_batch(*X.case_batch(c, c.B, s)) for s in range(3)]
        names = ["pi", "log_alpha"] + [f"qnet_{i}" for i in range(c.NC)] + [f"qnet_tgt_{i}" for i in range(c.NC)]
        out = {n: a.get_params(n) for n in names}
        for n in names:
            if n.startswith("qnet_tgt"): continue
            for role in ("exp_avg", "exp_avg_sq") + (() if n == "log_alpha" else ("grad",)):
                out[n + "/" + role] = a.get_params(n, role)
        out.update({k: a.probe(k, c.B) for k in a.PROBES})
        outs.append((out, recs))
        a.close()
    (f, frec), (u, urec) = outs
    assert frec == urec
    for k in f:
        assert np.array_equal(f[k].view(np.uint32), u[k].view(np.uint32)), k


def test_layer_probe_refuses_what_it_cannot_serve(B, monkeypatch):
    import ctypes as C
    from border_amd import _lib
    c = X.CASES["tiny-padded"]
    a = make_agent(B, c, monkeypatch)
    try:
        out = np.zeros(4096, np.float32)
        call = lambda ph, buf, i, l, n: _lib.lib().bdr_sac_layer_probe(a.handle, ph, buf, i, l, out.ctypes.data_as(C.c_void_p), n)
        assert call(1, a.BUFS["logp"], 0, 0, c.B) == 1                 # before any update
        a.update_on_batch(*X.case_batch(c, c.B, 0))
        assert call(1, a.BUFS["logp"], 0, 0, c.B) == 0
        assert call(0, a.BUFS["logp"], 0, 0, c.B) == 1                 # no snapshot: keep_layers is off
        a.keep_layers(True)
        a.update_on_batch(*X.case_batch(c, c.B, 1))
        assert call(0, a.BUFS["logp"], 0, 0, c.B) == 0
        assert call(2, a.BUFS["logp"], 0, 0, c.B) == 1                 # unknown phase
        assert call(1, 30, 0, 0, c.B) == 1 and call(1, -1, 0, 0, c.B) == 1   # unknown buffer
        assert call(1, a.BUFS["logp"], 0, 0, c.B + 1) == 1             # wrong float count
        assert call(1, a.BUFS["c_act"], 1, 0, c.B * 64) == 1           # critic out of range (NC = 1)
        assert call(1, a.BUFS["c_act"], 0, 2, c.B * 64) == 1           # layer out of range (two layers)
        assert call(1, a.BUFS["t_act"], 0, 1, c.B * 64) == 1           # trunk layer out of range
        assert call(1, a.BUFS["logp"], 0, 1, c.B) == 1                 # an index on a buffer that has none
        for buf in ("x_no", "xq_n", "xq_c", "tgt", "dxq"):              # not the actor phase's (dxq: the row-block kernels never form it)
            n = c.B if buf == "tgt" else c.B * 64
            assert call(0, a.BUFS[buf], 0, 0, n) == 1 and call(1, a.BUFS[buf], 0, 0, n) == 0, buf
    finally:
        a.close()
