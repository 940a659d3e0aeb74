"""Every kernel of the IQN step against an f64 evaluation of ITS OWN layer on the device's own inputs (tests/iqn_layer_reference.py).

tests/test_gpu_iqn.py sees what leaves the step (z, the loss, the flat gradient at 5e-4 of the arena's largest entry, norms at 1e-3)
- 100 to 1000 x above what these kernels can produce.  Here one update_on_batch runs with given percent points, Iqn.probe returns
every buffer the step left behind (padding included), and each output - cos, phi, the merge net's activations and z, tgt, every
weight / bias gradient, every dh, dlin, dpsi, the feature extractor's chain (Mlp, or the conv trunk behind k_reduce_partials) - is
compared with the f64 result of its own layer on the probed inputs.  ReLU masks come from the probed activations: NO element is exempt.
Per element, u = 2^-24, S = sum |a_k| |b_k|, n the reduction length:  (a) S == 0 -> exactly 0 (every padding column);
(b) |err| <= n u S;  (c) |err| <= lambda sqrt(n) u S with lambda = 4 x the sequential f32 restatement's largest ratio, floored at 1
(iqn_layer_reference.RESTATEMENT_RATIO, computed on the CPU, not fitted to the device); the split-operand kernels get SPLIT_C * S on
top of both (the module derives it).  The probes are taken BEFORE Iqn.forward fetches z_tgt (forward overwrites the buffers).

Cases (iqn_layer_reference.CASES; psi = Mlp(8 -> [64] -> F) unless cnn):
  tiny-padded    B=3 Np=9 Nt=100 F=100 E=48 units (96,) A=64, linear psi output: one tile nearly all padding; Fp, Ep, Np padding; 64 live lanes
                 and the wrapped n += 64 loop in k_iqn_target; mask_psi = 0.
  n33-chunked    B=65 Np=Nt=33 F=128 E=64 units (128,) A=6: M = 2145, 8 dW chunks of 9 ... 9, 5 tiles, the last tile one row, every sample
                 straddles tiles; then B=5 Np=9 Nt=5 on the same agent (capacity above batch, ch = 1 straight into grad).
  n10-chunked    B=256 Np=Nt=10 units (128, 64) A=9: M = 2560, groups of 10, dense_dx with i > 1, a chunked plain dense_dw.
  split-fused    B=64 Np=Nt=64 F=2048 E=64 units (512,) A=5 bf16x3_6: iqn_phi_3xbf16, f_fwd1_3xbf16, f_dw1_3xbf16, f_dx1_3xbf16 with the
                 merge epilogue; again with BDR_IQN_NO_MERGE_EPILOGUE=1; again with a linear psi output.  Labels asserted.
  split-n32      B=128 Np=Nt=32: iqn_merge_bwd behind dense_dx_b3, dense_dw_b3 with groups of 32.
  split-ragged   B=125 Np=Nt=33 E=100: M = 4125, ragged last 128-row tile in the split forward and dX; dw1_b3 off (M % 64), phi on
                 dense_forward (Ep = 128).  Labels asserted.
  exact          the split-fused shape with arithmetic="f32_exact".
  cnn-b3, cnn-b40  AtariCnn{skip_linear} trunk, units (64,), A=6: B=3 Np=9 Nt=5; B=40 Np=Nt=8 (both chunk caps of conv_dw_plan).
Acting (bdr_iqn_qvalues, Const32's 33 points, units (512,)): n = 1, 8 (ACT_SMALL_MAX: launch_act_layer<2>, <3> for conv2 / conv3 and
<1> for the merge layer), 9 (the convs on the training kernels - the psi_conv2 label appears -, the merge layer, M = 297 <= 512,
still launch_act_layer<1>), 16 (M = 528: everything on the training kernels).

Largest |err| / (sqrt(n) u S) per output (outputs of further merge-net layers share the row of layer 2: gWf3 -> gWf2): sequential f32
restatement on the CPU over every case | measured on an MI355X, the largest of the "iqn layer ratios" lines the tests print (all
cases, the follow-up update, the three split-fused variants, the four acting calls; for the split-operand outputs after SPLIT_C * S
is taken off) | lambda.  The device figures are a record, not a bar: if a later change fails (c) by a small factor, compare its
printed line with this first.  The device cosf stayed within 1.16 u of f64 cos of its own f32 argument (printed as "cosf ... u").
  cos   k_iqn_cos                                                  restatement 0.976 | MI355X 0.976 | lambda 3.90
  phi   dense_forward | dense_forward_k64_b3                       restatement 0.799 | MI355X 0.594 | lambda 3.20
  hf1   dense_forward_had | dense_forward_had_b3 | launch_act_layer<1> restatement 0.340 | MI355X 0.327 | lambda 1.36
  z     dense_forward                                              restatement 0.283 | MI355X 0.243 | lambda 1.13
  gWf2  dense_dw                                                   restatement 0.855 | MI355X 0.959 | lambda 3.42
  gbf2  dense_dw                                                   restatement 0.366 | MI355X 0.341 | lambda 1.46
  dhf1  dense_dx                                                   restatement 0.999 | MI355X 0.999 | lambda 4.00
  gWf1  dense_dw<Had> | dense_dw_b3                                restatement 1.192 | MI355X 1.287 | lambda 4.77
  gbf1  dense_dw<Had> | dense_dw_b3                                restatement 0.685 | MI355X 0.879 | lambda 2.74
  dlin  dense_dx | dense_dx_b3 + k_iqn_merge_bwd | dense_dx_had_b3 restatement 0.579 | MI355X 0.587 | lambda 2.32
  dpsi  dense_dx | dense_dx_b3 + k_iqn_merge_bwd | dense_dx_had_b3 restatement 0.185 | MI355X 0.185 | lambda 1.00
  gWc   dense_dw (cos layer)                                       restatement 1.748 | MI355X 1.505 | lambda 6.99
  gbc   dense_dw (cos layer)                                       restatement 1.166 | MI355X 1.152 | lambda 4.66
  gWp1  dense_dw                                                   restatement 1.337 | MI355X 1.172 | lambda 5.35
  gbp1  dense_dw                                                   restatement 1.019 | MI355X 1.050 | lambda 4.08
  dp0   dense_dx                                                   restatement 0.567 | MI355X 0.437 | lambda 2.27
  gWp0  dense_dw                                                   restatement 0.928 | MI355X 0.940 | lambda 3.71
  gbp0  dense_dw                                                   restatement 0.617 | MI355X 0.697 | lambda 2.47
  tgt   k_iqn_target                                               restatement 0.498 | MI355X 0.498 | lambda 1.99
  hf2   dense_forward                                              restatement 0.363 | MI355X 0.314 | lambda 1.45
  dhf2  dense_dx                                                   restatement 0.998 | MI355X 0.996 | lambda 3.99
  gW3   k_igemm_red<DwC3> + k_reduce_partials                      restatement 0.410 | MI355X 0.205 | lambda 1.64
  gb3   k_igemm_red<DwC3> + k_reduce_partials                      restatement 0.176 | MI355X 0.089 | lambda 1.00
  dy2   launch_igemm<DxC3Pos>                  restatement 0.398 | MI355X 0.306 | lambda 1.59
  gW2   k_igemm_red<DwC2> + k_reduce_partials                      restatement 0.300 | MI355X 0.179 | lambda 1.20
  gb2   k_igemm_red<DwC2> + k_reduce_partials                      restatement 0.080 | MI355X 0.056 | lambda 1.00
  dy1   launch_igemm<DxC2MPos>                 restatement 0.385 | MI355X 0.436 | lambda 1.54
  gW1   launch_conv1_dw_bf16 + k_reduce_partials                   restatement 0.135 | MI355X 0.084 | lambda 1.00
  gb1   launch_conv1_dw_bf16 + k_reduce_partials                   restatement 0.054 | MI355X 0.013 | lambda 1.00
  a2    conv2 forward                                              restatement 0.157 | MI355X 0.192 | lambda 1.00
  a3    conv3 forward                                              restatement 0.125 | MI355X 0.140 | lambda 1.00
  q     k_iqn_average                                              restatement 0.091 | MI355X 0.133 | lambda 1.00
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iqn_layer_reference as Q  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def make_agent(B, c, **kw):
    s = c.spec
    f_cfg = (B.AtariCnnConfig(n_stack=s.n_stack, skip_linear=True) if s.cnn else
             B.MlpConfig(in_dim=s.in_dim, units=tuple(s.psi_units), out_dim=s.F, activation_out=s.act_out))
    cfg = B.IqnConfig(f_config=f_cfg, feature_dim=s.F, embed_dim=s.E, m_units=tuple(s.m_units), n_actions=s.A, lr=1e-4, batch_size=c.B, device=0,
                      discount_factor=s.gamma, tau=1.0, soft_update_interval=10000, arithmetic=c.arithmetic, **kw)
    return B.Iqn.build(cfg)


def cosf_units(tau, cos_dev, E):
    """largest |cosf(x) - cos(x)| / u on the SAME f32 argument x (the record behind iqn_layer_reference.COSF_U)."""
    c, _ = Q.cos_args(tau, cos_dev.shape[1])
    arg = (np.asarray(tau, np.float32).reshape(-1, 1) * c[None, :]).astype(np.float32)
    return float(np.abs(cos_dev[:, :E].astype(np.float64) - np.cos(arg[:, :E].astype(np.float64))).max() / Q.U)


def probe_forward(a, spec, n, N, inp):
    M = n * N
    L = len(spec.m_units) + 1
    inp.update(cos=a.probe("cos", M), phi=a.probe("phi", M), psi=a.probe("psi", n), f_act=[a.probe("f_act", M, i) for i in range(L)])
    if spec.cnn:
        inp.update(a1=a.probe("a1", n).reshape(n, 20, 20, 32), a2=a.probe("a2", n).reshape(n, 9, 9, 64))
    else:
        inp["x_in"] = Q._padded(np.asarray(inp["obs"], np.float32), (n, Q.pad64(spec.in_dim)))
        inp["psi_act"] = [a.probe("psi_act", n, j) for j in range(len(spec.psi_units) + 1)]
    return inp


def forward_dev(inp):
    L = len(inp["f_act"])
    dev = {"cos": inp["cos"], "phi": inp["phi"], "z": inp["f_act"][-1]}
    dev.update({"hf%d" % (i + 1): inp["f_act"][i] for i in range(L - 1)})
    return dev


def assert_not_vacuous(inp, c):
    both = lambda x: (np.asarray(x) == 0).any() and (np.asarray(x) > 0).any()
    s = c.spec
    assert both(inp["phi"][:, :s.F]) and all(both(h[:, :u]) for h, u in zip(inp["f_act"], s.m_units)), "a vacuous case"
    assert (inp["psi"] > 0).any() and (not s.mask_psi or both(inp["psi"][:, :s.F]))
    assert ((inp["f_dy"][-1] != 0).sum(1) == 1).all(), "every row of dz has one nonzero"
    act = inp["act"]
    assert Q.EMPTY_ACTION not in act and len(set(act.tolist())) == min(c.B, s.A - 1) and inp["term"].any() and not inp["term"].all()


def update_and_check(a, c, label, merge_epilogue=True, labels_want=None):
    p0, p_tgt = Q.case_params(c)
    a.set_params(p0, "iqn"); a.set_params(p_tgt, "iqn_tgt")
    batch = Q.case_batch(c)
    obs, act, nobs, rew, term, tau_p, tau_t = batch
    s, M = c.spec, c.B * c.Np
    L = len(s.m_units) + 1
    a.update_on_batch(*batch)
    inp = dict(spec=s, P=Q.internal_params(p0, s), tau=tau_p, obs=obs, act=act, rew=rew, term=term)    # p0: BEFORE the optimizer step
    probe_forward(a, s, c.B, c.Np, inp)
    inp.update(f_dy=[a.probe("f_dy", M, i) for i in range(L)], dlin=a.probe("dlin", M), dpsi=a.probe("dpsi", c.B))
    tgt_dev = a.probe("tgt", c.B, cols=c.Nt)
    if s.cnn:
        inp.update(dy2=a.probe("dy2", c.B).reshape(c.B, 9, 9, 64), dy1=a.probe("dy1", c.B).reshape(c.B, 20, 20, 32))
    else:
        inp["psi_dy"] = [a.probe("psi_dy", c.B, j) for j in range(len(s.psi_units) + 1)]
    grads = a.get_params("grad")
    inp["z_tgt"] = a.forward(nobs, tau_t, "iqn_tgt")          # after every probe: it overwrites the buffers
    ok, gap = Q.tgt_gap_ok(inp["z_tgt"])
    assert ok, "the argmax of a row's mean could depend on the summation order: gap / threshold %.3g" % gap
    assert_not_vacuous(inp, c)
    dev = forward_dev(inp)
    dev.update({"dhf%d" % i: inp["f_dy"][i - 1] for i in range(1, L)})
    dev.update(dlin=inp["dlin"], dpsi=inp["dpsi"], tgt=tgt_dev)
    if s.cnn:
        dev.update(dy2=inp["dy2"], dy1=inp["dy1"])
    else:
        dev.update({"dp%d" % j: inp["psi_dy"][j] for j in range(len(s.psi_units))})
    dev.update(Q.device_grads(grads, s))
    ops = Q.reference(inp, split=Q.split_outputs(c, merge_epilogue))
    assert set(ops) == set(dev), set(ops) ^ set(dev)
    ratios = Q.sharp_ratios(ops, dev)
    print("iqn layer ratios %s: cosf %.2f u | " % (label, cosf_units(tau_p, inp["cos"], s.E)) + " ".join("%s %.3f" % (k, ratios[k]) for k in ops))
    Q.check_all(ops, dev, Q.LAMBDA)


def run_case(B, name, label=None, merge_epilogue=True, want=(), absent=(), follow_up=None):
    import bench
    c = Q.CASES[name]
    a = make_agent(B, c)
    try:
        a.profile_enable(True)
        update_and_check(a, c, label or name, merge_epilogue)
        labels = [l for l, _ in bench.read_profile(a)]
        a.profile_enable(False)
        assert all(l in labels for l in want) and not any(l in labels for l in absent), labels
        if follow_up:
            update_and_check(a, Q.CASES[follow_up], "%s then %s" % (name, follow_up))
    finally:
        a.close()


@pytest.fixture(autouse=True)
def _no_ab_switches(monkeypatch):
    for v in ("BDR_IQN_F32_EXACT", "BDR_IQN_NO_MERGE_EPILOGUE", "BDR_IQN_PHI_F32", "BDR_IQN_DW_F32"):
        monkeypatch.delenv(v, raising=False)


SPLIT = ("iqn_f_fwd1_3xbf16", "iqn_f_dx1_3xbf16")


def test_tiny_padded(B):
    run_case(B, "tiny-padded", want=("iqn_phi", "iqn_f_fwd1", "iqn_merge_bwd"))


def test_n33_chunked_then_a_smaller_batch(B):
    assert Q.dw_chunks(65 * 33) == 8 and (65 * 33) % 32 == 1
    run_case(B, "n33-chunked", want=("iqn_f_dw1", "iqn_merge_bwd"), follow_up="n33-follow-up")


def test_n10_chunked_two_hidden_layers(B):
    run_case(B, "n10-chunked", want=("iqn_f_dw2", "iqn_f_dx2", "iqn_f_dw3"))


@pytest.mark.parametrize("variant", ["fused", "separate-merge", "linear-psi"])
def test_split_fused(B, monkeypatch, variant):
    if variant == "separate-merge":
        monkeypatch.setenv("BDR_IQN_NO_MERGE_EPILOGUE", "1")
    sep = variant == "separate-merge"
    run_case(B, "split-fused-linear-psi" if variant == "linear-psi" else "split-fused", "split-fused " + variant, merge_epilogue=not sep,
             want=SPLIT + ("iqn_phi_3xbf16", "iqn_f_dw1_3xbf16") + (("iqn_merge_bwd",) if sep else ()), absent=() if sep else ("iqn_merge_bwd",))


def test_split_n32(B):
    run_case(B, "split-n32", want=SPLIT + ("iqn_phi_3xbf16", "iqn_f_dw1_3xbf16", "iqn_merge_bwd"))


def test_split_ragged(B):
    assert (125 * 33) % 128 != 0 and (125 * 33) % 64 != 0
    run_case(B, "split-ragged", want=SPLIT + ("iqn_phi", "iqn_f_dw1", "iqn_merge_bwd"), absent=("iqn_phi_3xbf16", "iqn_f_dw1_3xbf16"))


def test_exact_control(B):
    run_case(B, "exact", want=("iqn_phi", "iqn_f_fwd1", "iqn_f_dw1", "iqn_f_dx1", "iqn_merge_bwd"), absent=SPLIT + ("iqn_phi_3xbf16", "iqn_f_dw1_3xbf16"))


@pytest.mark.parametrize("name", ["cnn-b3", "cnn-b40"])
def test_cnn_trunk(B, name):
    run_case(B, name, want=("psi_conv3_dw", "psi_conv2_dw", "psi_conv1_dw"))


@pytest.mark.parametrize("n", [1, 8, 9, 16])
def test_acting_forward(B, n):
    """qvalues on n observations: a2, a3, cos, phi, h, z each against f64 of its own layer on the probed input, q = mean_n z."""
    import bench
    from oracle import torch_ref as T
    s = Q.Spec(kind="cnn", F=3136, E=64, m_units=(512,), A=6)
    c = Q.Case("acting", s, n, 33, 33, 21, 0)
    p0 = T.init_params(s.shapes(), 21)
    a = make_agent(B, c)
    try:
        a.set_params(p0, "iqn")
        obs = np.random.default_rng(50 + n).integers(0, 256, (n, 4, 1, 84, 84), dtype=np.uint8)
        a.profile_enable(True)
        q = a.qvalues(obs)
        labels = [l for l, _ in bench.read_profile(a)]
        a.profile_enable(False)
        assert ("psi_conv2" in labels) == (n > 8), labels      # <= ACT_SMALL_MAX: launch_act_layer<2> / <3>, no trunk bracket
        tau = np.tile((np.arange(33, dtype=np.float32) * np.float32(1.0 / 32.0))[None], (n, 1))
        inp = probe_forward(a, s, n, 33, dict(spec=s, P=Q.internal_params(p0, s), tau=tau, obs=obs))
    finally:
        a.close()
    ops = Q.forward_ops(inp)
    ops.update(Q.conv_forward_ops(inp))
    ops["q"] = Q.q_op(inp["f_act"][-1].reshape(n, 33, -1), s.A)
    dev = forward_dev(inp)
    dev.update(a2=inp["a2"], a3=inp["psi"].reshape(n, 7, 7, 64), q=q)
    assert all((np.asarray(dev[k]) > 0).any() and (np.asarray(dev[k]) == 0).any() for k in ("a2", "a3", "phi", "hf1"))
    ratios = Q.sharp_ratios(ops, dev)
    print("iqn layer ratios acting n=%d: cosf %.2f u | " % (n, cosf_units(tau, inp["cos"], s.E)) + " ".join("%s %.3f" % (k, ratios[k]) for k in ops))
    Q.check_all(ops, dev, Q.LAMBDA)


def test_probe_refuses_what_it_cannot_serve(B):
    """An unknown `what`, a probe before any forward, a gradient probe before any update and a wrong float count are errors of the library."""
    from border_amd import _lib
    import ctypes as C
    c = Q.CASES["n33-follow-up"]
    a = make_agent(B, c)
    try:
        with pytest.raises(_lib.BdrError, match="nothing to probe yet"):
            a.probe("phi", c.B * c.Np)
        a.forward(Q.case_batch(c)[0], Q.case_batch(c)[5], "iqn")
        assert a.probe("phi", c.B * c.Np).shape == (45, 128)
        with pytest.raises(_lib.BdrError, match="no update has run"):
            a.probe("dlin", c.B * c.Np)
        with pytest.raises(_lib.BdrError, match="floats, not"):
            a.probe("phi", c.B * c.Np + 1)
        out = np.zeros(4, np.float32)
        assert _lib.lib().bdr_iqn_probe(a.handle, 11, out.ctypes.data_as(C.c_void_p), 4) == 1      # BDR_ERR_INVALID
        assert _lib.lib().bdr_iqn_probe(a.handle, 16 + 5, out.ctypes.data_as(C.c_void_p), 4) == 1
        with pytest.raises(_lib.BdrError):
            a.probe("a1", c.B)                                                                     # Mlp feature extractor
    finally:
        a.close()
