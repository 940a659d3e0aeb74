"""Float64 reference, float32 restatement and cases of the IQN step's kernels, one layer at a time (csrc/iqn.hip model_forward /
update_critic).  Written beside tests/dqn_backward_reference.py, whose Op, check, check_all, sharp_ratios and conv operations it uses.
Nothing under border_amd/ imports this file.

Given the device's own inputs of a kernel (Iqn.probe: cos, phi, psi, every hidden activation and z, every dy, dlin, dpsi, the trunk's
buffers; the parameters and percent points the test set) each output is a sum of products accumulated in f32, so it can differ from
the f64 evaluation of the same sum only by the roundings of the accumulation - plus, for the split-operand kernels, the three
partial products they drop.

  reference(inp, split)   per output an Op: f64 result `ref`, S = sum |a_k| |b_k|, reduction length n (terms whose dy factor is
                          exactly 0 are not counted: they add nothing), and where the output is not a bare reduction an absolute
                          allowance `extra` that check() takes off |err| first.  ReLU masks come from the probed post-activations
                          (`> 0`, as the epilogues do): no element is exempt.  The Hadamard operand m = phi[m] * psi[m / N] is formed as
                          the device forms it, ONE f32 multiply (numpy float32: IEEE gives the same bits), and enters the sums as an
                          exact input.  Arrays keep the device's padded leading dimensions and the parameters are zero-padded, so a
                          padding column has S == 0 and criterion (a) demands that it is exactly 0.
  restatement(inp, mutate) the same operations in float32 with sequential accumulation; sets lambda, and with `mutate` is the wrong kernel
                          of the host self-test (tests/test_iqn_layer_reference.py).
  criteria                (a) S == 0 -> exactly 0;  (b) |err| <= n u S;  (c) |err| <= lambda sqrt(n) u S, u = 2^-24.

Bounds that are not a bare reduction
  cos    cosv[m][i] = cosf(fl(tau * c_i)), c_i = fl(pi_f32 * (i + 1)) (k_iqn_cos; both multiplies are f32, nothing can be contracted).
         Against cos(tau * c_i) with the product exact: the rounded argument is off by <= u |arg| and |sin| <= 1, so that is
         <= u |arg|; plus the device cosf's own error.  The ROCm toolchain ships no statement of that error (the device library
         comes as bitcode without an accuracy table), so it was measured: against f64 cos of the SAME f32 argument, over every case's cos
         probe on an MI355X, the largest |cosf(x) - cos(x)| is COSF_MEASURED_U = 1.16 units of u = 2^-24 (x in [0, 64 pi]); the bar
         COSF_U = 2 is that figure rounded up to the next whole unit.  Op: S = |arg| + COSF_U, n = 1.
  split  igemm_b3.hpp split3_rn: x = t0 + t1 + t2 exactly, each term the round-to-nearest bf16 (8 significant bits) of what is left.
         With 2^e <= |x| < 2^(e+1): |t0| <= 2^(e+1), |r1| = |x - t0| <= 2^(e-8) (half a spacing of 2^(e-7)), so |t1| <= 2^(e-8); unless r1 is
         exactly 2^(e-8) (then t2 = 0) its exponent is <= e - 9 and |t2| = |r1 - t1| <= 2^(e-17).  The 6-term kernels (TERMS = 6 in
         dense.hpp: launch_igemm_b3<.., 6>, k_igemm_red_b3<6>, dense_k64_b3.hpp) drop t1 u2, t2 u1 and t2 u2 of a product x y:
         <= (2^-25 + 2^-25 + 2^-34) |x| |y|.  SPLIT_C = 2^-24 + 2^-34 per product, i.e. SPLIT_C * S per output, a worst case.
         (tests/test_gpu_dqn.py quotes 3 * 2^-26 for the same split: that is the size when every residual is half its maximum, not a
         bound; the code gives the figure above.)  extra += SPLIT_C * S on the outputs in `split`.
  dlin   dm = dy1 W1 is not observable (dense_dx / dense_dx_b3 leave it in `mrg`, k_iqn_merge_bwd or the dense_dx_had_b3 epilogue
         overwrite it).  dm carries its GEMM's bound e_dm (n u S_dm, or lambda sqrt(n) u S_dm); dlin = 1{phi > 0} fl(dm psi):
         |err| <= |psi| e_dm + u |dm psi|.   Op: S = |psi| S_dm, n of dm, extra = u |dm psi|.
  dpsi   = 1{psi > 0 | no output ReLU} sum_n dm_n phi_n in f32 (an fmaf chain of N terms, or the epilogue's tree):
         |err| <= sum_n |phi_n| e_dm,n + (N + 1) u sum_n |dm_n phi_n|.   Op: S = sum_n |phi_n| S_dm,n, extra = (N + 1) u sum_n |dm_n phi_n|.
  tgt    k_iqn_target: the argmax over f32 means accumulated in row order (restated exactly; the cases keep every row's top-two gap
         100 x above Nt u sum |z|, asserted by tgt_gap_ok, so no summation order can change it), then r + k z with k = fl((1 - term)
         gamma): one fma or a multiply and an add, <= 2 u (|r| + |k z|).   Op: S = 2 (|r| + |k z|), n = 1.
  q      k_iqn_average: (sum_n z) / N in f32: <= (N + 1) u sum |z| / N.   Op: S = (N + 1) sum |z| / N, n = 1.

Layouts are the device's: rows m = b * N + n; the feature axis of phi / psi / dlin / dpsi is the device's (for the AtariCnn trunk
position-major, hw * 64 + c; internal_params permutes the reference's channel-major cos and merge weights to it, as Iqn::to_internal
does); weights here are [out][in], zero-padded to multiples of 64."""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_backward_reference as R  # noqa: E402
from dqn_backward_reference import Op, U, check, check_all, sharp_ratios  # noqa: E402,F401

SPLIT_C = 2.0 ** -24 + 2.0 ** -34
COSF_MEASURED_U = 1.16     # largest over every case of tests/test_gpu_iqn_layers.py on an MI355X (its printed "cosf ... u")
COSF_U = 2.0
PI_F32 = np.float32(3.14159265358979323846)


def pad64(x: int) -> int:
    return (x + 63) // 64 * 64


@dataclass(frozen=True)
class Spec:
    kind: str = "mlp"                    # "mlp": Mlp(in_dim -> psi_units -> F) | "cnn": AtariCnn{skip_linear}
    F: int = 128
    E: int = 64
    m_units: Sequence[int] = (128,)
    A: int = 6
    in_dim: int = 8
    psi_units: Sequence[int] = (64,)
    act_out: bool = True                 # MlpConfig::activation_out of psi (the cnn trunk always ends in a ReLU)
    n_stack: int = 4
    gamma: float = 0.99

    @property
    def cnn(self):
        return self.kind == "cnn"

    @property
    def mask_psi(self):
        return self.cnn or self.act_out

    def shapes3(self):
        from oracle import torch_ref as T
        return T.iqn_shapes(self.kind, self.F, self.E, list(self.m_units), self.A, psi_in=self.in_dim, psi_units=list(self.psi_units), n_stack=self.n_stack)

    def shapes(self):
        a, b, c = self.shapes3()
        return a + b + c

    def fperm(self):
        """reference feature j -> the device's feature index (Iqn::fperm)."""
        j = np.arange(self.F)
        return (j % 49) * 64 + j // 49 if self.cnn else j


def _padded(a, shape):
    out = np.zeros(shape, np.float32)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


def internal_params(flat, spec: Spec) -> dict:
    """A flat vector in reference order (parameters, or the gradient arena from get_params) -> psi: [(W, b)] of the Mlp or the six
    conv arrays in reference shapes; Wc [Fp][Ep], bc [Fp]; f: [(W [Np][Kp], b [Np])], the first with its inputs in device order."""
    ts, o = [], 0
    for s in spec.shapes():
        n = int(np.prod(s)); ts.append(np.asarray(flat[o:o + n], np.float32).reshape(s)); o += n
    n_psi = len(spec.shapes3()[0])
    fp, Fp, Ep = spec.fperm(), pad64(spec.F), pad64(spec.E)
    P = {}
    if spec.cnn:
        P["conv"] = ts[:6]
    else:
        P["psi"] = [(_padded(ts[i], (pad64(ts[i].shape[0]), pad64(ts[i].shape[1]))), _padded(ts[i + 1], (pad64(ts[i].shape[0]),))) for i in range(0, n_psi, 2)]
    Wc, bc = np.zeros((spec.F, spec.E), np.float32), np.zeros(spec.F, np.float32)
    Wc[fp], bc[fp] = ts[n_psi], ts[n_psi + 1]
    P["Wc"], P["bc"] = _padded(Wc, (Fp, Ep)), _padded(bc, (Fp,))
    P["f"] = []
    for k, i in enumerate(range(n_psi + 2, len(ts), 2)):
        W = ts[i]
        if k == 0:
            Wd = np.zeros_like(W); Wd[:, fp] = W; W = Wd
        P["f"].append((_padded(W, (pad64(W.shape[0]), pad64(W.shape[1]))), _padded(ts[i + 1], (pad64(W.shape[0]),))))
    return P


def device_grads(flat, spec: Spec) -> dict:
    """The gradient arena (get_params("grad")) -> the outputs' names."""
    G = internal_params(flat, spec)
    out = {"gWc": G["Wc"], "gbc": G["bc"]}
    for i, (W, b) in enumerate(G["f"]):
        out["gWf%d" % (i + 1)], out["gbf%d" % (i + 1)] = W, b
    if spec.cnn:
        for k, name in enumerate(("gW1", "gb1", "gW2", "gb2", "gW3", "gb3")):
            out[name] = G["conv"][k]
    else:
        for i, (W, b) in enumerate(G["psi"]):
            out["gWp%d" % i], out["gbp%d" % i] = W, b
    return out


# ------------------------------------------------------------------------------------------------ f64 reference
def _d(x):
    return np.asarray(x, np.float64)


def _count(dy, axis):
    """terms that can add anything: the nonzero entries of dy along `axis` (at least 1)."""
    return np.maximum((np.asarray(dy) != 0).sum(axis), 1).astype(np.float64)


def _op(name, kern, ref, S, n, extra=None):
    ref = np.asarray(ref, np.float64)
    return Op(name, ref, np.asarray(S, np.float64), np.broadcast_to(np.asarray(n, np.float64), ref.shape), None,
              None if extra is None else np.asarray(extra, np.float64), kern)


def had_rows(phi, psi, N):
    """m = phi[m] * psi[m / N] as ONE float32 multiply (the A operand of the merge layer's forward and weight gradient)."""
    return np.asarray(phi, np.float32) * np.repeat(np.asarray(psi, np.float32)[:, :phi.shape[1]], N, axis=0)


def cos_args(tau, Ep):
    """fl(pi_f32 * (i + 1)) for i < Ep, and the exact products tau * c_i in f64."""
    c = (PI_F32 * np.arange(1, Ep + 1, dtype=np.float32)).astype(np.float32)
    return c, _d(np.asarray(tau, np.float32).reshape(-1, 1)) * _d(c)[None, :]


def _fwd(x, W, b, n_in, relu):
    x, W, b = _d(x), _d(W), _d(b)
    ref = x @ W.T + b
    S = np.abs(x) @ np.abs(W).T + np.abs(b)
    return (np.maximum(ref, 0) if relu else ref), S, n_in + 1


def _dw(x, dy):
    x, dy = _d(x), _d(dy)
    return dy.T @ x, np.abs(dy).T @ np.abs(x), _count(dy, 0)


def _dx(dy, W, mask):
    dyd, W = _d(dy), _d(W)
    ref, S = dyd @ W, np.abs(dyd) @ np.abs(W)
    if mask is not None:
        m = np.asarray(mask) > 0
        ref, S = ref * m, S * m
    return ref, S, _count(dy, 1)[:, None]


KERN = {
    "cos": "k_iqn_cos", "phi": "dense_forward | dense_forward_k64_b3", "hf1": "dense_forward_had | dense_forward_had_b3 | launch_act_layer<1>",
    "dlin": "dense_dx | dense_dx_b3 + k_iqn_merge_bwd | dense_dx_had_b3", "dpsi": "dense_dx | dense_dx_b3 + k_iqn_merge_bwd | dense_dx_had_b3",
    "gWc": "dense_dw (cos layer)", "gbc": "dense_dw (cos layer)", "gWf1": "dense_dw<Had> | dense_dw_b3", "gbf1": "dense_dw<Had> | dense_dw_b3",
    "tgt": "k_iqn_target", "q": "k_iqn_average", "a2": "conv2 forward", "a3": "conv3 forward",
}
SPLITTABLE = ("phi", "hf1", "gWf1", "gbf1", "dlin", "dpsi")


def _kern(name):
    if name in KERN: return KERN[name]
    if name.startswith("hf") or name == "z": return "dense_forward"
    if name.startswith(("gWf", "gbf", "gWp", "gbp")): return "dense_dw"
    if name.startswith(("dhf", "dp")): return "dense_dx"
    return R.KERNEL[name] + (" + k_reduce_partials" if name.startswith("g") else "")


def forward_ops(inp: dict, split=()) -> dict:
    """cos, phi, hf1 .. hf{L-1}, z from the probed inputs of each layer (tau; cos; phi and psi; the activation before)."""
    spec, P = inp["spec"], inp["P"]
    N = inp["tau"].shape[1]
    Ep = P["Wc"].shape[1]
    out = {}
    _, arg = cos_args(inp["tau"], Ep)
    live = (np.arange(Ep) < spec.E)[None, :]
    out["cos"] = _op("cos", KERN["cos"], np.cos(arg) * live, (np.abs(arg) + COSF_U) * live, 1.0)
    ref, S, n = _fwd(inp["cos"], P["Wc"], P["bc"], spec.E, True)
    out["phi"] = _op("phi", KERN["phi"], ref, S, n)
    x = had_rows(inp["phi"], inp["psi"], N)
    L = len(P["f"])
    for i, (W, b) in enumerate(P["f"]):
        name = "z" if i == L - 1 else "hf%d" % (i + 1)
        ref, S, n = _fwd(x, W, b, spec.F if i == 0 else spec.m_units[i - 1], i < L - 1)
        out[name] = _op(name, _kern(name), ref, S, n)
        x = inp["f_act"][i]
    for k in split:
        if k in out: out[k].extra = SPLIT_C * out[k].S
    return out


def backward_ops(inp: dict, split=()) -> dict:
    """Every gradient from the probed dy of its layer: gWf / gbf / dhf of the merge net, dlin, dpsi, gWc, gbc, the Mlp feature
    extractor's chain or the conv trunk's (dqn_backward_reference's operations on dy3 = dpsi, a2, a1, obs)."""
    spec, P = inp["spec"], inp["P"]
    N = inp["tau"].shape[1]
    L = len(P["f"])
    out = {}
    x1 = had_rows(inp["phi"], inp["psi"], N)
    for i in range(L - 1, -1, -1):
        x = x1 if i == 0 else inp["f_act"][i - 1]
        dy = inp["f_dy"][i]
        ref, S, n = _dw(x, dy)
        out["gWf%d" % (i + 1)] = _op("gWf%d" % (i + 1), _kern("gWf%d" % (i + 1)), ref, S, n[:, None])
        out["gbf%d" % (i + 1)] = _op("gbf%d" % (i + 1), _kern("gbf%d" % (i + 1)), _d(dy).sum(0), np.abs(_d(dy)).sum(0), n)
        if i > 0:
            ref, S, n = _dx(dy, P["f"][i][0], inp["f_act"][i - 1])
            out["dhf%d" % i] = _op("dhf%d" % i, "dense_dx", ref, S, n)
    dm, S_dm, n_dm = _dx(inp["f_dy"][0], P["f"][0][0], None)
    Fp = dm.shape[1]
    B = inp["psi"].shape[0]
    psi = _d(inp["psi"])[:, :Fp]
    psi_rep, phi = np.repeat(psi, N, axis=0), _d(inp["phi"])
    live = phi > 0
    out["dlin"] = _op("dlin", KERN["dlin"], dm * psi_rep * live, np.abs(psi_rep) * S_dm * live, n_dm, U * np.abs(dm * psi_rep) * live)
    pm = (psi > 0) if spec.mask_psi else np.ones_like(psi, bool)
    grp = lambda a: a.reshape(B, N, Fp).sum(1)
    ref, S, ex = grp(dm * phi) * pm, grp(np.abs(phi) * S_dm) * pm, (N + 1) * U * grp(np.abs(dm * phi)) * pm
    ldf = inp["psi"].shape[1]
    wide = lambda a: np.pad(a, ((0, 0), (0, ldf - Fp)))
    out["dpsi"] = _op("dpsi", KERN["dpsi"], wide(ref), wide(S), n_dm.reshape(B, N).max(1)[:, None], wide(ex))
    ref, S, n = _dw(inp["cos"], inp["dlin"])
    out["gWc"] = _op("gWc", KERN["gWc"], ref, S, n[:, None])
    out["gbc"] = _op("gbc", KERN["gbc"], _d(inp["dlin"]).sum(0), np.abs(_d(inp["dlin"])).sum(0), n)
    if spec.cnn:
        names = ("gW3", "gb3", "dy2", "gW2", "gb2", "dy1", "gW1", "gb1")
        c = P["conv"]
        z = lambda *s: np.zeros(s, np.float32)
        fake = dict(params=list(c) + [z(512, 3136), z(512), z(spec.A, 512), z(spec.A)], obs=inp["obs"], act=np.zeros(B, np.int64),
                    a1=inp["a1"], a2=inp["a2"], a3=np.asarray(inp["psi"]).reshape(B, 7, 7, 64), h1=z(B, 512), dq=z(B), dh1=z(B, 512),
                    dy3=np.asarray(inp["dpsi"]).reshape(B, 7, 7, 64), dy2=inp["dy2"], dy1=inp["dy1"])
        for k, op in R.reference(fake, only=names).items():
            op.kern = R.KERNEL[k] + (" + k_reduce_partials" if k.startswith("g") else "")
            out[k] = op
    else:
        PL = len(P["psi"])
        for j in range(PL - 1, -1, -1):
            x = inp["x_in"] if j == 0 else inp["psi_act"][j - 1]
            dy = inp["psi_dy"][j]
            ref, S, n = _dw(x, dy)
            out["gWp%d" % j] = _op("gWp%d" % j, "dense_dw", ref, S, n[:, None])
            out["gbp%d" % j] = _op("gbp%d" % j, "dense_dw", _d(dy).sum(0), np.abs(_d(dy)).sum(0), n)
            if j > 0:
                ref, S, n = _dx(dy, P["psi"][j][0], inp["psi_act"][j - 1])
                out["dp%d" % (j - 1)] = _op("dp%d" % (j - 1), "dense_dx", ref, S, n)
    for k in split:
        if k in out:
            out[k].extra = SPLIT_C * out[k].S + (0 if out[k].extra is None else out[k].extra)
    return out


def target_choice(z_tgt, last_point=False):
    """k_iqn_target's action: f32 means accumulated in row order, the first of equal maxima.  Returns (action [B], mean [B][A])."""
    z = np.asarray(z_tgt, np.float32)
    s = np.zeros((z.shape[0], z.shape[2]), np.float32)
    for n in range(z.shape[1]):
        s = s + z[:, n]
    mean = s / np.float32(z.shape[1])
    return (z[:, -1] if last_point else mean).argmax(1), mean


def tgt_gap_ok(z_tgt):
    """Every row's top-two gap of the mean is more than 100 x Nt u sum |z| (the largest any f32 summation order can move a mean's
    sum, divided through by Nt on both sides): the argmax cannot depend on the order.  Returns (ok, smallest gap / threshold)."""
    z = _d(z_tgt)
    Nt = z.shape[1]
    top = np.sort(z.mean(1), axis=1)[:, -2:]
    thr = 100.0 * Nt * U * np.abs(z).sum(1).max(1) / Nt
    r = (top[:, 1] - top[:, 0]) / thr
    return bool((r > 1).all()), float(r.min())


def target_op(z_tgt, rew, term, gamma) -> Op:
    a, _ = target_choice(z_tgt)
    zs = _d(np.take_along_axis(np.asarray(z_tgt, np.float32), a[:, None, None], 2)[:, :, 0])
    k = _d((np.float32(1) - np.asarray(term, np.float32)) * np.float32(gamma))[:, None]
    r = _d(np.asarray(rew, np.float32))[:, None]
    return _op("tgt", KERN["tgt"], r + k * zs, 2 * (np.abs(r) + np.abs(k * zs)), 1.0)


def q_op(z, A) -> Op:
    """z [n][N][ldz] (the probed rows) -> q [n][A]."""
    z = _d(z)[:, :, :A]
    N = z.shape[1]
    return _op("q", KERN["q"], z.mean(1), (N + 1) * np.abs(z).sum(1) / N, 1.0)


def conv_forward_ops(inp: dict) -> dict:
    """a2, a3 of the trunk from the probed a1 / a2 and the conv parameters (acting calls): relu(conv + bias), n = taps + 1."""
    c = inp["P"]["conv"]
    out = {}
    for name, x, W, b, st in (("a2", inp["a1"], c[2], c[3], 2), ("a3", inp["a2"], c[4], c[5], 1)):
        xt, Wt, bt = R._nchw(R._t(x)), R._t(W), R._t(b)
        ref = R._nhwc(F.conv2d(xt, Wt, bt, stride=st)).numpy()
        S = R._nhwc(F.conv2d(xt.abs(), Wt.abs(), bt.abs(), stride=st)).numpy()
        out[name] = _op(name, KERN[name], np.maximum(ref, 0), S, float(W[0].size + 1))
    return out


def seq_conv_forward(x_nhwc, W, b, stride):
    """relu(conv + bias) in sequential f32 over the im2col taps."""
    cols = R._cols(x_nhwc, W.shape[2], stride)
    B, H = x_nhwc.shape[0], (x_nhwc.shape[1] - W.shape[2]) // stride + 1
    return _seq_fwd(cols.astype(np.float32), np.asarray(W, np.float32).reshape(W.shape[0], -1), b, True).reshape(B, H, H, W.shape[0])


def seq_average(z, A):
    z = np.asarray(z, np.float32)[:, :, :A]
    s = np.zeros((z.shape[0], A), np.float32)
    for n in range(z.shape[1]):
        s = s + z[:, n]
    return s / np.float32(z.shape[1])


def acting_ratios(n: int) -> dict:
    """a2, a3, q of an acting call on n observations (the cnn agent of tests/test_gpu_iqn_layers.py::test_acting_forward), restated."""
    from oracle import torch_ref as T
    s = Spec(kind="cnn", F=3136, E=64, m_units=(512,), A=6)
    P = internal_params(T.init_params(s.shapes(), 21), s)
    obs = np.random.default_rng(50 + n).integers(0, 256, (n, 4, 1, 84, 84), dtype=np.uint8)
    tau = np.tile((np.arange(33, dtype=np.float32) * np.float32(1.0 / 32.0))[None], (n, 1))
    inp = dict(spec=s, P=P, tau=tau, **_f32_forward(s, P, obs, tau))
    ops = conv_forward_ops(inp)
    ops["q"] = q_op(inp["f_act"][-1].reshape(n, 33, -1), s.A)
    c = P["conv"]
    val = dict(a2=seq_conv_forward(inp["a1"], c[2], c[3], 2), a3=seq_conv_forward(inp["a2"], c[4], c[5], 1), q=seq_average(inp["f_act"][-1].reshape(n, 33, -1), s.A))
    return sharp_ratios(ops, val)


def reference(inp: dict, split=()) -> dict:
    out = forward_ops(inp, split)
    out.update(backward_ops(inp, split))
    if "z_tgt" in inp:
        out["tgt"] = target_op(inp["z_tgt"], inp["rew"], inp["term"], inp["spec"].gamma)
    return out


# ------------------------------------------------------------------------------------------------ float32 restatement
_acc = R._acc


def _seq_fwd(x, W, b, relu, had_shift=None, psi=None, phi=None, N=None):
    """bias + sum_k x[:, k] W[:, k] in f32, k ascending.  had_shift = b: the first row of sample b takes psi of sample b - 1."""
    if had_shift is not None:
        x = np.array(x, np.float32)
        m = had_shift * N
        x[m] = np.asarray(phi, np.float32)[m] * np.asarray(psi, np.float32)[had_shift - 1, :x.shape[1]]
    x64, W64 = _d(x), _d(W)
    acc = np.zeros((x64.shape[0], W64.shape[0]), np.float32)
    for k in np.flatnonzero((np.abs(W64).sum(0) > 0) & (np.abs(x64).sum(0) > 0)):
        acc = _acc(acc, x64[:, k:k + 1] * W64[:, k][None, :])
    acc = _acc(acc, np.broadcast_to(_d(b)[None, :], acc.shape))
    return np.maximum(acc, np.float32(0)) if relu else acc


def _seq_dw(x, dy, drop_rows=None):
    """sum_m dy[m][:, None] x[m][None, :] in f32, m ascending -> ([Np][Kp], [Np]).  drop_rows = (lo, hi): rows left out."""
    x64, dy64 = _d(x), _d(dy)
    gw, gb = np.zeros((dy64.shape[1], x64.shape[1]), np.float32), np.zeros(dy64.shape[1], np.float32)
    lo, hi = drop_rows if drop_rows else (0, 0)
    for m in range(x64.shape[0]):
        if lo <= m < hi or not dy64[m].any(): continue
        gw = _acc(gw, dy64[m][:, None] * x64[m][None, :])
        gb = _acc(gb, dy64[m])
    return gw, gb


def _seq_dx(dy, W, mask):
    dy64, W64 = _d(dy), _d(W)
    acc = np.zeros((dy64.shape[0], W64.shape[1]), np.float32)
    for j in np.flatnonzero(np.abs(dy64).sum(0)):
        acc = _acc(acc, dy64[:, j:j + 1] * W64[j][None, :])
    return acc if mask is None else np.where(np.asarray(mask) > 0, acc, np.float32(0))


def seq_target(z_tgt, rew, term, gamma, last_point=False, tail_unwritten=False):
    a, _ = target_choice(z_tgt, last_point)
    zs = np.take_along_axis(np.asarray(z_tgt, np.float32), a[:, None, None], 2)[:, :, 0]
    k = ((np.float32(1) - np.asarray(term, np.float32)) * np.float32(gamma))[:, None]
    t = (_d(np.asarray(rew, np.float32))[:, None] + _d(k) * _d(zs)).astype(np.float32)     # one fma
    if tail_unwritten: t[:, 64:] = 0
    return t


def restatement(inp: dict, only=None, mutate: Optional[dict] = None) -> dict:
    """The outputs of reference() in sequential float32.  mutate: {output: keyword arguments}: drop_rows (gW*), had_shift (hf1, gWf1),
    mask=False (dlin: phi > 0; dpsi: psi > 0), pad_nonzero (phi), last_point / tail_unwritten (tgt)."""
    mut = mutate or {}
    spec, P = inp["spec"], inp["P"]
    N = inp["tau"].shape[1]
    L = len(P["f"])
    want = (lambda k: True) if only is None else (lambda k: k in only)
    g = lambda k: np.asarray(inp[k], np.float32)
    out = {}
    if want("cos"):
        c, _ = cos_args(inp["tau"], P["Wc"].shape[1])
        arg = (np.asarray(inp["tau"], np.float32).reshape(-1, 1) * c[None, :]).astype(np.float32)
        out["cos"] = np.where(np.arange(c.size)[None, :] < spec.E, np.cos(_d(arg)).astype(np.float32), np.float32(0))
    if want("phi"):
        out["phi"] = _seq_fwd(g("cos"), P["Wc"], P["bc"], True)
        if "pad_nonzero" in mut.get("phi", {}): out["phi"][0, spec.F + mut["phi"]["pad_nonzero"]] = np.float32(1e-30)
    x1 = had_rows(g("phi"), g("psi"), N)
    x = x1
    for i, (W, b) in enumerate(P["f"]):
        name = "z" if i == L - 1 else "hf%d" % (i + 1)
        if want(name):
            m = mut.get(name, {})
            out[name] = _seq_fwd(x, W, b, i < L - 1, psi=g("psi"), phi=g("phi"), N=N, **m) if i == 0 else _seq_fwd(x, W, b, i < L - 1)
        x = inp["f_act"][i]
    for i in range(L - 1, -1, -1):
        nw, nb = "gWf%d" % (i + 1), "gbf%d" % (i + 1)
        if want(nw) or want(nb):
            m = dict(mut.get(nw, {}))
            xi = x1 if i == 0 else inp["f_act"][i - 1]
            if i == 0 and "had_shift" in m:
                b_ = m.pop("had_shift")
                xi = xi.copy(); xi[b_ * N] = g("phi")[b_ * N] * g("psi")[b_ - 1, :xi.shape[1]]
            out[nw], out[nb] = _seq_dw(xi, inp["f_dy"][i], **m)
        if i > 0 and want("dhf%d" % i):
            out["dhf%d" % i] = _seq_dx(inp["f_dy"][i], P["f"][i][0], inp["f_act"][i - 1])
    if want("dlin") or want("dpsi"):
        dm = _seq_dx(inp["f_dy"][0], P["f"][0][0], None)
        Fp, B, ldf = dm.shape[1], inp["psi"].shape[0], inp["psi"].shape[1]
        psi, phi = g("psi")[:, :Fp], g("phi")
        v = (dm * np.repeat(psi, N, axis=0)).astype(np.float32)
        out["dlin"] = np.where(phi > 0, v, np.float32(0)) if mut.get("dlin", {}).get("mask", True) else v
        s = np.zeros((B, Fp), np.float32)
        d3, p3 = _d(dm).reshape(B, N, Fp), _d(phi).reshape(B, N, Fp)
        for n in range(N):
            s = _acc(s, d3[:, n] * p3[:, n])
        if spec.mask_psi and mut.get("dpsi", {}).get("mask", True):
            s = np.where(psi > 0, s, np.float32(0))
        out["dpsi"] = np.pad(s, ((0, 0), (0, ldf - Fp)))
    if want("gWc") or want("gbc"):
        out["gWc"], out["gbc"] = _seq_dw(g("cos"), g("dlin"), **mut.get("gWc", {}))
    if spec.cnn:
        names = tuple(k for k in ("gW3", "gb3", "dy2", "gW2", "gb2", "dy1", "gW1", "gb1") if want(k))
        if names:
            B = inp["psi"].shape[0]
            fake = dict(params=list(P["conv"]) + [None] * 2 + [np.zeros((spec.A, 512), np.float32), None], obs=inp["obs"], act=np.zeros(B, np.int64),
                        a1=inp["a1"], a2=inp["a2"], dy3=g("dpsi").reshape(B, 7, 7, 64), dy2=inp["dy2"], dy1=inp["dy1"])
            out.update(R.restatement(fake, only=names, mutate={k: v for k, v in mut.items() if k in names}))
    else:
        for j in range(len(P["psi"]) - 1, -1, -1):
            if want("gWp%d" % j) or want("gbp%d" % j):
                out["gWp%d" % j], out["gbp%d" % j] = _seq_dw(inp["x_in"] if j == 0 else inp["psi_act"][j - 1], inp["psi_dy"][j], **mut.get("gWp%d" % j, {}))
            if j > 0 and want("dp%d" % (j - 1)):
                out["dp%d" % (j - 1)] = _seq_dx(inp["psi_dy"][j], P["psi"][j][0], inp["psi_act"][j - 1])
    if "z_tgt" in inp and want("tgt"):
        out["tgt"] = seq_target(inp["z_tgt"], inp["rew"], inp["term"], spec.gamma, **mut.get("tgt", {}))
    return {k: v for k, v in out.items() if want(k)}


# ------------------------------------------------------------------------------------------------ inputs without a device
def _f32_forward(spec: Spec, P, obs, tau):
    """The buffers a forward leaves behind, from a float32 evaluation on the CPU (torch): what the device would probe, up to summation
    order."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    B, N = tau.shape
    r = {}
    if spec.cnn:
        c = [t(a) for a in P["conv"]]
        x = t(np.asarray(obs).reshape(B, -1, 84, 84)) / 255
        a1 = F.conv2d(x, c[0], c[1], stride=4).relu(); a2 = F.conv2d(a1, c[2], c[3], stride=2).relu(); a3 = F.conv2d(a2, c[4], c[5], stride=1).relu()
        r["a1"], r["a2"] = (R._nhwc(a).contiguous().numpy() for a in (a1, a2))
        r["psi"] = R._nhwc(a3).contiguous().numpy().reshape(B, 3136)
    else:
        x = t(_padded(np.asarray(obs, np.float32), (B, pad64(spec.in_dim))))
        r["x_in"], r["psi_act"] = x.numpy(), []
        for j, (W, b) in enumerate(P["psi"]):
            x = F.linear(x, t(W), t(b))
            if j < len(P["psi"]) - 1 or spec.act_out: x = x.relu()
            r["psi_act"].append(x.numpy())
        r["psi"] = r["psi_act"][-1]
    c, _ = cos_args(tau, P["Wc"].shape[1])
    arg = (np.asarray(tau, np.float32).reshape(-1, 1) * c[None, :]).astype(np.float32)
    r["cos"] = np.where(np.arange(c.size)[None, :] < spec.E, np.cos(arg), np.float32(0)).astype(np.float32)
    r["phi"] = F.linear(t(r["cos"]), t(P["Wc"]), t(P["bc"])).relu().numpy()
    x = t(had_rows(r["phi"], r["psi"], N))
    r["f_act"] = []
    for i, (W, b) in enumerate(P["f"]):
        x = F.linear(x, t(W), t(b))
        if i < len(P["f"]) - 1: x = x.relu()
        r["f_act"].append(x.numpy())
    return r


def loss_dz(z, act, tau_p, tgt):
    """k_iqn_loss's dz rows [M][ldz] in float32 (the loss kernel itself is covered by tests/edge_inputs.py; here it is an input)."""
    z, tgt, tau_p = np.asarray(z, np.float32), np.asarray(tgt, np.float32), np.asarray(tau_p, np.float32)
    B, Np = tau_p.shape
    Nt = tgt.shape[1]
    pred = z.reshape(B, Np, -1)[np.arange(B)[:, None], np.arange(Np)[None, :], np.asarray(act)[:, None]]
    d = tgt[:, None, :] - pred[:, :, None]                                   # [B][Np][Nt]
    dh = np.where(np.abs(d) < 1, d, np.sign(d)).astype(np.float32)
    w = np.abs(tau_p[:, :, None] - (d < 0).astype(np.float32))
    gsum = -(w * dh).sum(2, dtype=np.float32) * (np.float32(1) / (np.float32(B) * np.float32(Nt) * np.float32(Np)))
    dz = np.zeros_like(z).reshape(B, Np, -1)
    dz[np.arange(B)[:, None], np.arange(Np)[None, :], np.asarray(act)[:, None]] = gsum
    return dz.reshape(z.shape)


def cpu_inputs(spec: Spec, p_flat, p_tgt_flat, batch, restate_chain=True) -> dict:
    """The inputs of reference() / restatement() for one update, without a device: forward buffers from _f32_forward, tgt and dz from
    the float32 formulas, and the chain of gradient intermediates each from the restatement of the kernel that produces it."""
    obs, act, nobs, rew, term, tau_p, tau_t = batch
    P, Pt = internal_params(p_flat, spec), internal_params(p_tgt_flat, spec)
    B, Np = tau_p.shape
    inp = dict(spec=spec, P=P, tau=np.asarray(tau_p, np.float32), obs=np.asarray(obs), act=np.asarray(act, np.int64),
               rew=np.asarray(rew, np.float32), term=np.asarray(term, np.int8))
    zt = _f32_forward(spec, Pt, nobs, np.asarray(tau_t, np.float32))["f_act"][-1]
    inp["z_tgt"] = zt.reshape(B, tau_t.shape[1], -1)[:, :, :spec.A].copy()
    inp.update(_f32_forward(spec, P, obs, inp["tau"]))
    inp["tgt"] = seq_target(inp["z_tgt"], rew, term, spec.gamma)
    L = len(P["f"])
    inp["f_dy"] = [None] * L
    inp["f_dy"][L - 1] = loss_dz(inp["f_act"][-1], act, tau_p, inp["tgt"])
    if restate_chain:
        fill_chain(inp)
    return inp


def fill_chain(inp):
    spec, P = inp["spec"], inp["P"]
    L = len(P["f"])
    for i in range(L - 1, 0, -1):
        inp["f_dy"][i - 1] = _seq_dx(inp["f_dy"][i], P["f"][i][0], inp["f_act"][i - 1])
    r = restatement(inp, only=("dlin", "dpsi"))
    inp["dlin"], inp["dpsi"] = r["dlin"], r["dpsi"]
    if spec.cnn:
        B = inp["psi"].shape[0]
        fake = dict(params=list(P["conv"]), a1=inp["a1"], a2=inp["a2"], dy3=inp["dpsi"].reshape(B, 7, 7, 64))
        fake["dy2"] = R._seq_dx(fake["dy3"], P["conv"][4], inp["a2"], 1, 9)
        fake["dy1"] = R._seq_dx(fake["dy2"], P["conv"][2], inp["a1"], 2, 20)
        inp["dy2"], inp["dy1"] = fake["dy2"], fake["dy1"]
    else:
        PL = len(P["psi"])
        inp["psi_dy"] = [None] * PL
        inp["psi_dy"][PL - 1] = inp["dpsi"]
        for j in range(PL - 1, 0, -1):
            inp["psi_dy"][j - 1] = _seq_dx(inp["psi_dy"][j], P["psi"][j][0], inp["psi_act"][j - 1])


# ------------------------------------------------------------------------------------------------ the test cases
@dataclass(frozen=True)
class Case:
    name: str
    spec: Spec
    B: int
    Np: int
    Nt: int
    seed: int
    tgt_seed: int                      # seed of the target network's parameters, chosen by `python tests/iqn_layer_reference.py seeds` so that tgt_gap_ok holds
    arithmetic: str = "bf16x3_6"
    small: bool = True                 # cheap enough for the host self-test to restate


_MLP = dict(kind="mlp", in_dim=8, psi_units=(64,))
_BIG = Spec(F=2048, E=64, m_units=(512,), A=5, **_MLP)
CASES = {c.name: c for c in (
    Case("tiny-padded", Spec(F=100, E=48, m_units=(96,), A=64, act_out=False, **_MLP), 3, 9, 100, 11, 0),
    Case("n33-chunked", Spec(F=128, E=64, m_units=(128,), A=6, **_MLP), 65, 33, 33, 12, 0, small=False),
    Case("n33-follow-up", Spec(F=128, E=64, m_units=(128,), A=6, **_MLP), 5, 9, 5, 13, 0),
    Case("n10-chunked", Spec(F=128, E=64, m_units=(128, 64), A=9, **_MLP), 256, 10, 10, 14, 0, small=False),
    Case("split-fused", _BIG, 64, 64, 64, 15, 0, small=False),
    Case("split-fused-linear-psi", Spec(F=2048, E=64, m_units=(512,), A=5, act_out=False, **_MLP), 64, 64, 64, 15, 0, small=False),
    Case("split-n32", _BIG, 128, 32, 32, 16, 0, small=False),
    Case("split-ragged", Spec(F=2048, E=100, m_units=(512,), A=5, **_MLP), 125, 33, 33, 17, 1, small=False),
    Case("exact", _BIG, 64, 64, 64, 15, 0, arithmetic="f32_exact", small=False),
    Case("cnn-b3", Spec(kind="cnn", F=3136, E=64, m_units=(64,), A=6), 3, 9, 5, 18, 0),
    Case("cnn-b40", Spec(kind="cnn", F=3136, E=64, m_units=(64,), A=6), 40, 8, 8, 19, 0, small=False),
)}
EMPTY_ACTION = 0      # the action no row of a case takes


def case_batch(c: Case):
    """oracle.torch_ref.iqn_batch with the actions spread: action 0 has no rows, every other action has one as far as the rows go
    (tiny-padded has 3 rows for 64 actions), in shuffled row order; row 0 is terminated, row 1 is not."""
    from oracle import torch_ref as T
    s = c.spec
    obs, act, nobs, rew, term, tp, tt = T.iqn_batch(c.B, s.kind, s.A, c.Np, c.Nt, c.seed + 100, in_dim=s.in_dim, n_stack=s.n_stack)
    act = (1 + np.arange(c.B) % (s.A - 1))[np.random.default_rng(c.seed).permutation(c.B)].astype(np.int64)
    term = term.copy(); term[0] = 1
    if c.B > 1: term[1] = 0
    return obs, act, nobs, rew, term, tp, tt


def case_params(c: Case):
    from oracle import torch_ref as T
    sh = c.spec.shapes()
    return T.init_params(sh, c.seed), T.init_params(sh, 1000 * (c.tgt_seed + 1) + c.seed)


def uses_b3(c: Case) -> bool:
    """Iqn::use_b3 for the case's update."""
    s, M = c.spec, c.B * c.Np
    Kp, Np1 = pad64(s.F), pad64(s.m_units[0])
    return c.arithmetic == "bf16x3_6" and Np1 % 128 == 0 and Kp * Np1 >= 1 << 20 and M >= 4096


def dw_chunks(M: int) -> int:
    return 1 if M <= 2048 else min(32, (M // 1024 + 7) // 8 * 8)


def split_outputs(c: Case, merge_epilogue=True) -> tuple:
    """The outputs that the split-operand kernels produce in this case (the conditions of csrc/iqn.hip), and the labels to expect."""
    if not uses_b3(c):
        return ()
    M = c.B * c.Np
    out = ["hf1", "dlin", "dpsi"]
    if pad64(c.spec.E) == 64: out.append("phi")
    if M % 64 == 0 and c.Np % 8 == 0 and dw_chunks(M) > 1: out += ["gWf1", "gbf1"]
    return tuple(out)


# Criterion (c)'s factor per output: 4 x the largest |err| / (sqrt(n) u S) of the sequential float32 restatement against f64 over
# the cases above (`python tests/iqn_layer_reference.py` prints a line per case and the "largest:" line this table is a copy of, to three decimals; the
# activations come from cpu_inputs), floored at 1.  The 4 is for the device's accumulation order.  NOT fitted to the device.
# tests/test_iqn_layer_reference.py recomputes the small cases' rows.
RESTATEMENT_RATIO = {
    'cos': 0.976, 'phi': 0.799, 'hf1': 0.340, 'z': 0.283, 'gWf2': 0.855, 'gbf2': 0.366, 'dhf1': 0.999, 'gWf1': 1.192, 'gbf1': 0.685, 'dlin': 0.579,
    'dpsi': 0.185, 'gWc': 1.748, 'gbc': 1.166, 'gWp1': 1.337, 'gbp1': 1.019, 'dp0': 0.567, 'gWp0': 0.928, 'gbp0': 0.617, 'tgt': 0.498, 'hf2': 0.363,
    'dhf2': 0.998, 'gW3': 0.410, 'gb3': 0.176, 'dy2': 0.398, 'gW2': 0.300, 'gb2': 0.080, 'dy1': 0.385, 'gW1': 0.135, 'gb1': 0.054,
    'a2': 0.157, 'a3': 0.125, 'q': 0.091}   # the last three: the "acting n=" lines (bdr_iqn_qvalues on 1 and 9 observations)
# the largest over the small cases alone (tiny-padded, n33-follow-up, cnn-b3): what the host self-test can recompute in seconds
RESTATEMENT_SMALL = {
    'cos': 0.913, 'phi': 0.387, 'hf1': 0.314, 'z': 0.187, 'gWf2': 0.795, 'gbf2': 0.366, 'dhf1': 0.986, 'gWf1': 1.192, 'gbf1': 0.685, 'dlin': 0.392,
    'dpsi': 0.052, 'gWc': 1.583, 'gbc': 1.166, 'gWp1': 1.215, 'gbp1': 0.751, 'dp0': 0.287, 'gWp0': 0.928, 'gbp0': 0.617, 'tgt': 0.448, 'gW3': 0.410,
    'gb3': 0.176, 'dy2': 0.398, 'gW2': 0.300, 'gb2': 0.080, 'dy1': 0.322, 'gW1': 0.135, 'gb1': 0.054}


def lam_of(name: str) -> float:
    return max(1.0, 4.0 * RESTATEMENT_RATIO.get(_family(name), 0.25))


def _family(name: str) -> str:
    """Outputs share a table row per kernel family and layer kind (gWf2, gWf3 -> gWf2: the plain dense_dw)."""
    for pre in ("gWf", "gbf", "dhf", "hf"):
        if name.startswith(pre) and name[len(pre):].isdigit() and int(name[len(pre):]) > 2:
            return pre + "2"
    return name


class _Lam(dict):
    def __missing__(self, k):
        return lam_of(k)


LAMBDA = _Lam()


def case_ratios(c: Case) -> dict:
    p, pt = case_params(c)
    inp = cpu_inputs(c.spec, p, pt, case_batch(c))
    ops = reference(inp)
    val = restatement(inp)
    return {_family(k): v for k, v in sharp_ratios(ops, {k: val[k] for k in ops}).items()}


if __name__ == "__main__":
    sys.path.insert(0, __file__.rsplit("/tests/", 1)[0])
    if sys.argv[1:] == ["seeds"]:
        import dataclasses
        for c in CASES.values():
            for ts in range(200):
                c2 = dataclasses.replace(c, tgt_seed=ts)
                _, pt = case_params(c2)
                b = case_batch(c2)
                zt = _f32_forward(c.spec, internal_params(pt, c.spec), b[2], b[6])["f_act"][-1].reshape(c.B, c.Nt, -1)[:, :, :c.spec.A]
                ok, r = tgt_gap_ok(zt)
                if ok and r > 3: break
            print("%s tgt_seed %d gap ratio %.2f" % (c.name, ts, r), flush=True)
        sys.exit(0)
    names = sys.argv[1:] or list(CASES)
    worst = {}
    for nm in names:
        r = case_ratios(CASES[nm])
        print(nm + ": " + " ".join("%s %.3f" % kv for kv in r.items()), flush=True)
        for k, v in r.items(): worst[k] = max(worst.get(k, 0.0), v)
    if not sys.argv[1:]:
        for n in (1, 9):
            r = acting_ratios(n)
            print("acting n=%d: " % n + " ".join("%s %.3f" % kv for kv in r.items()), flush=True)
            for k, v in r.items(): worst[k] = max(worst.get(k, 0.0), v)
    print("largest: " + " ".join("'%s': %.3f," % kv for kv in worst.items()))
