"""Float64 reference, float32 restatement and checker of the CNN DQN step's backward kernels, one layer at a time.
Nothing under border_amd/ imports this file.

Every kernel of the backward pass (csrc/dqn.hip update_critic) is a sum of EXACT products accumulated in f32: the dX and dW GEMMs run
on the FP32 MFMA, conv1's dW multiplies u8 pixels with an exact three-term bf16 split of dy1, the head kernels are fmaf chains.  So
given the device's own inputs of a kernel (Dqn.probe: activations, h1, dq, dh1, dy3, dy2, dy1; the parameters the test set), its
output can differ from the f64 evaluation of the same sum only by the roundings of the accumulation.

  reference(inp)        per output an Op: the f64 result `ref`, S = sum |a_k| |b_k| (the same operation on absolute values) and the
                        reduction length `n` per element.  ReLU masks are taken from the probed activation (`> 0`, as the kernels'
                        epilogues do), so no unit can be masked differently by reference and device: no element is exempt.
  restatement(inp)      the same operations in float32 with SEQUENTIAL accumulation in row order (numpy; each product is formed
                        exactly, in f64, and added into an f32 accumulator - what an fmaf chain or an MFMA step does).  It sets the
                        scale of criterion (c) and is the "correct kernel" of the host self-test; `drop_row`, `drop_tap`, ... make it
                        wrong on purpose.
  check(op, dev, lam)   (a) where S == 0 the device value is exactly 0 (masked units, actions without rows);
                        (b) |dev - ref| <= n u S, u = 2^-24: holds for exact products summed in f32 in any order (to first order in u);
                        (c) |dev - ref| <= lam sqrt(n) u S: the sharp bound - one lost or doubled term is ~|a b| ~ S / n, far above it.

Layouts are the device's: activations and dy* position-major ([B][H][W][C]); parameters and the gradient arena in the reference's
variable order (c1.weight [32][ns][8][8] ... l1.weight [512][3136] with the 3136 inputs channel-major (c, h, w), l2.weight [A][512]).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
INV255_F32 = np.float32(1.0) / np.float32(255.0)

# kernel (csrc/dqn.hip update_critic) that produces each output
KERNEL = {
    "dh1": "k_head (TD part)", "gW5": "k_head_bwd", "gb5": "k_head_bwd",
    "gW4": "k_igemm_red<DwL1>", "gb4": "k_igemm_red<DwL1>", "dy3": "launch_igemm<DxL1>",
    "gW3": "k_igemm_red<DwC3>", "gb3": "k_igemm_red<DwC3>", "dy2": "launch_igemm<DxC3Pos>",
    "gW2": "k_igemm_red<DwC2>", "gb2": "k_igemm_red<DwC2>", "dy1": "launch_igemm<DxC2MPos>",
    "gW1": "launch_conv1_dw_bf16", "gb1": "launch_conv1_dw_bf16",
}
# outputs that pass through the partial-sum reduction of k_reduce_adam before they reach the gradient arena
REDUCED = ("gW1", "gb1", "gW2", "gb2", "gW3", "gb3")
# position in the gradient arena (reference variable order)
GRAD_INDEX = {"gW1": 0, "gb1": 1, "gW2": 2, "gb2": 3, "gW3": 4, "gb3": 5, "gW4": 6, "gb4": 7, "gW5": 8, "gb5": 9}
OPS = tuple(KERNEL)

# Criterion (c)'s factor per output: 4 x the largest |err| / (sqrt(n) u S) that the sequential float32 restatement reaches against
# f64 on the inputs of the six test cases (RESTATEMENT_RATIO: `python tests/dqn_backward_reference.py` prints them; activations from
# a CPU evaluation of the same parameters and batches), floored at 1.  The 4 is for the device's accumulation order (k = 2 MFMA steps,
# chunk partials, fixed-order combine) - it is NOT fitted to the device.  Where n is small (dh1: 1, the head and l1 gradients: the
# rows of an action, B) sqrt(n) is close to n and (b) is the binding bound anyway.
# The table is a record of that script's "largest:" line, to three decimals.  tests/test_dqn_backward_reference.py recomputes the
# B = 1, 3 and 7 rows (which set nine of the fourteen entries) and fails if CASES, the seeds or the restatement move away from it;
# after such a change run the script again and copy its line here.
RESTATEMENT_RATIO = {"dh1": 0.999, "gW5": 1.396, "gb5": 0.649, "gW4": 1.343, "gb4": 1.016, "dy3": 0.202, "gW3": 0.444, "gb3": 0.190,
                     "dy2": 0.402, "gW2": 0.466, "gb2": 0.163, "dy1": 0.448, "gW1": 0.212, "gb1": 0.080}
LAMBDA = {k: max(1.0, 4.0 * v) for k, v in RESTATEMENT_RATIO.items()}


def taps_c3(i: int) -> int:
    """Valid taps along one axis of conv3's input gradient (3x3, stride 1, 9 -> 7) at input coordinate i: 1, 2 or 3."""
    return sum(1 for k in range(3) if 0 <= i - k <= 6)


def taps_c2(i: int) -> int:
    """Valid taps along one axis of conv2's input gradient (4x4, stride 2, 20 -> 9) at input coordinate i: 1 or 2."""
    return sum(1 for k in range(4) if (i - k) % 2 == 0 and 0 <= (i - k) // 2 <= 8)


@dataclass
class Op:
    name: str
    ref: np.ndarray            # f64
    S: np.ndarray              # f64, same shape
    n: np.ndarray              # reduction length per element (broadcast to ref's shape)
    where: Optional[Callable[[tuple], str]] = None   # index of an element -> description (position-class kernels)
    # an absolute allowance per element that is taken off |err| before (b) and (c) are applied: roundings that do not belong to the
    # reduction (tests/iqn_layer_reference.py: the dropped partial products of the split-operand kernels, the multiply behind a GEMM).
    # It is 0 wherever S is 0, so (a) stands as it is.  None (every DQN output): nothing is taken off.
    extra: Optional[np.ndarray] = None
    kern: Optional[str] = None   # the producing kernel, for outputs that are not in KERNEL

    @property
    def kernel(self) -> str:
        return self.kern if self.kern is not None else KERNEL[self.name]


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).double()


def _nchw(x):   # [B][H][W][C] -> [B][C][H][W]
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def _dw(x_nchw, dy_nchw, k, stride):
    """Weight gradient of a valid conv: sum over (b, position) of unfold(x) * dy -> [cout][cin*k*k] in (cin, kh, kw) order."""
    B = x_nchw.shape[0]
    cols = F.unfold(x_nchw, k, stride=stride)                       # [B][cin*k*k][P]
    return torch.einsum("bop,bkp->ok", dy_nchw.reshape(B, dy_nchw.shape[1], -1), cols)


def _eval(inp: dict, absolute: bool) -> dict:
    """Every backward output in f64 from the device's own inputs; with `absolute`, the same sums over absolute values (S)."""
    f = (lambda x: x.abs()) if absolute else (lambda x: x)
    w = [f(_t(p)) for p in inp["params"]]            # c1.w c1.b c2.w c2.b c3.w c3.b l1.w l1.b l2.w l2.b
    W2, W3, W4, W5 = w[2], w[4], w[6], w[8]
    act = torch.from_numpy(np.asarray(inp["act"], np.int64))
    B, A = act.shape[0], W5.shape[0]
    obs = _t(np.asarray(inp["obs"]).reshape(B, -1, 84, 84))          # 0..255, never negative
    a1, a2, a3, h1 = (_t(inp[k]) for k in ("a1", "a2", "a3", "h1"))  # post-ReLU: never negative
    dq, dh1, dy3, dy2, dy1 = (f(_t(inp[k])) for k in ("dq", "dh1", "dy3", "dy2", "dy1"))
    onehot = F.one_hot(act, A).double()                              # [B][A]
    out = {}
    out["dh1"] = (h1 > 0) * (dq[:, None] * W5[act])
    out["gW5"] = onehot.t() @ (h1 * dq[:, None])
    out["gb5"] = onehot.t() @ dq
    a3f = _nchw(a3).reshape(B, 3136)                                 # l1's input: channel-major flatten
    out["gW4"] = dh1.t() @ a3f
    out["gb4"] = dh1.sum(0)
    out["dy3"] = (a3 > 0) * _nhwc((dh1 @ W4).reshape(B, 64, 7, 7))
    out["gW3"] = _dw(_nchw(a2), _nchw(dy3), 3, 1).reshape(64, 64, 3, 3)
    out["gb3"] = dy3.sum((0, 1, 2))
    out["dy2"] = (a2 > 0) * _nhwc(F.conv_transpose2d(_nchw(dy3), W3, stride=1))
    out["gW2"] = _dw(_nchw(a1), _nchw(dy2), 4, 2).reshape(64, 32, 4, 4)
    out["gb2"] = dy2.sum((0, 1, 2))
    out["dy1"] = (a1 > 0) * _nhwc(F.conv_transpose2d(_nchw(dy2), W2, stride=2))
    out["gW1"] = _dw(obs, _nchw(dy1), 8, 4).reshape(32, -1, 8, 8) / 255.0
    out["gb1"] = dy1.sum((0, 1, 2))
    return {k: v.numpy() for k, v in out.items()}


def _lengths(inp: dict) -> dict:
    act = np.asarray(inp["act"], np.int64)
    B, A = act.shape[0], np.asarray(inp["params"][8]).shape[0]
    rows = np.bincount(act, minlength=A).astype(np.float64)
    t3 = np.array([taps_c3(i) for i in range(9)], np.float64)
    t2 = np.array([taps_c2(i) for i in range(20)], np.float64)
    one = np.float64(1)
    return {
        "dh1": one, "gW5": rows[:, None], "gb5": rows, "gW4": one * B, "gb4": one * B, "dy3": one * 512,
        "gW3": one * B * 49, "gb3": one * B * 49, "dy2": (64 * np.outer(t3, t3))[None, :, :, None],
        "gW2": one * B * 81, "gb2": one * B * 81, "dy1": (64 * np.outer(t2, t2))[None, :, :, None],
        "gW1": one * (B * 400 + 1), "gb1": one * B * 400,            # + 1: the rounding of the 1/255 scale
    }


def _where_dy2(idx):
    b, ih, iw, c = idx
    return "tap class %d x %d = %d taps, image %d, position (%d, %d), channel %d" % (taps_c3(ih), taps_c3(iw), taps_c3(ih) * taps_c3(iw), b, ih, iw, c)


def _where_dy1(idx):
    b, ih, iw, c = idx
    return ("tap class %d x %d = %d taps, parity class (%d, %d), image %d, position (%d, %d) (half-resolution (%d, %d)), channel %d"
            % (taps_c2(ih), taps_c2(iw), taps_c2(ih) * taps_c2(iw), ih % 2, iw % 2, b, ih, iw, ih // 2, iw // 2, c))


def reference(inp: dict, only=None) -> dict:
    """name -> Op for the fourteen outputs (or those in `only`).  The weight and bias gradients (GRAD_INDEX) read no parameter: with
    `only=tuple(GRAD_INDEX)` the values in `params` do not matter (their shapes do).  inp: params (list of ten arrays in reference shapes, BEFORE the optimizer step), obs u8
    [B][ns][84][84] (an extra unit axis is accepted), act i64 [B], a1 [B][20][20][32], a2 [B][9][9][64], a3 [B][7][7][64], h1 [B][512],
    dq [B], dh1 [B][512], dy3 / dy2 / dy1 shaped like a3 / a2 / a1."""
    ref, S, n = _eval(inp, False), _eval(inp, True), _lengths(inp)
    where = {"dy2": _where_dy2, "dy1": _where_dy1}
    return {k: Op(k, ref[k], S[k], np.broadcast_to(n[k], ref[k].shape), where.get(k)) for k in (OPS if only is None else only)}


# ------------------------------------------------------------------------------------------------ checker
@dataclass
class Verdict:
    name: str
    kernel: str
    n_nonzero_where_zero: int      # (a)
    n_over_worst: int              # (b)
    n_over_sharp: int              # (c)
    worst_ratio: float             # max |err| / (n u S)
    sharp_ratio: float             # max |err| / (sqrt(n) u S)
    elements: int
    message: str

    @property
    def ok(self) -> bool:
        return self.n_nonzero_where_zero == 0 and self.n_over_worst == 0 and self.n_over_sharp == 0


def check(op: Op, dev, lam: float) -> Verdict:
    dev = np.asarray(dev, np.float64).reshape(op.ref.shape)
    err = np.abs(dev - op.ref)
    if op.extra is not None:
        err = np.maximum(err - op.extra, 0.0)
    zero = op.S == 0
    a_bad = zero & (dev != 0)
    scale, n = np.where(zero, 1.0, U * op.S), np.where(zero, 1.0, op.n)
    r_worst = np.where(zero, 0.0, err / (n * scale))
    r_sharp = np.where(zero, 0.0, err / (np.sqrt(n) * scale))
    if not np.isfinite(dev).all():
        r_worst = np.where(np.isfinite(dev), r_worst, np.inf); r_sharp = np.where(np.isfinite(dev), r_sharp, np.inf)
    b_bad, c_bad = r_worst > 1.0, r_sharp > lam
    msg = ""
    if a_bad.any() or b_bad.any() or c_bad.any():
        k = np.unravel_index(int(np.argmax(a_bad)) if a_bad.any() else int(np.argmax(r_sharp)), op.ref.shape)
        parts = []
        if a_bad.any(): parts.append("(a) %d elements with S == 0 are not exactly 0" % a_bad.sum())
        if b_bad.any(): parts.append("(b) %d elements above n u S (largest %.3g x)" % (b_bad.sum(), r_worst.max()))
        if c_bad.any(): parts.append("(c) %d elements above %.3g sqrt(n) u S (largest ratio %.3g)" % (c_bad.sum(), lam, r_sharp.max()))
        loc = op.where(tuple(int(i) for i in k)) if op.where else "index %s" % (tuple(int(i) for i in k),)
        msg = ("%s [%s], %d elements: %s; worst element: %s, device %.9g, f64 %.9g, S %.3g, n %d"
               % (op.kernel, op.name, err.size, "; ".join(parts), loc, dev[k], op.ref[k], op.S[k], int(op.n[k])))
    return Verdict(op.name, op.kernel, int(a_bad.sum()), int(b_bad.sum()), int(c_bad.sum()), float(r_worst.max()), float(r_sharp.max()), err.size, msg)


def check_all(ops: dict, dev: dict, lam: dict) -> dict:
    """Verdicts of every output in `dev`; raises one AssertionError that names every failing kernel."""
    v = {k: check(ops[k], dev[k], lam[k]) for k in dev}
    bad = [x.message for x in v.values() if not x.ok]
    assert not bad, "\n".join(bad)
    return v


# ------------------------------------------------------------------------------------------------ float32 restatement
def _acc(acc, prod64):
    """acc (f32) + an exact product (f64 holds f32 x f32 exactly), rounded to f32: one fmaf."""
    return (acc.astype(np.float64) + prod64).astype(np.float32)


def _seq_dw(x_rows, dy_rows, skip=None, rows=None, twice=None):
    """sum_m x[m][:, None] * dy[m][None, :] in f32, sequentially in row order -> [K][N] (last row of K: the bias column sums when x
    carries a column of ones).  skip: a row left out; rows: (lo, hi) only; twice: (lo, hi) rows whose partial is added a second time."""
    x64, dy64 = x_rows.astype(np.float64), dy_rows.astype(np.float64)
    lo, hi = rows if rows else (0, x64.shape[0])
    acc = np.zeros((x64.shape[1], dy64.shape[1]), np.float32)
    for m in range(lo, hi):
        if m != skip:
            acc = _acc(acc, x64[m][:, None] * dy64[m][None, :])
    if twice:
        acc = _acc(acc, _seq_dw(x_rows, dy_rows, rows=twice).astype(np.float64))
    return acc


def _cols(x_nhwc_or_nchw, k, stride, nchw=False):
    """im2col rows [B*P][cin*k*k] in (cin, kh, kw) order, f32-exact values."""
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc_or_nchw)).double()
    if not nchw: x = _nchw(x)
    c = F.unfold(x, k, stride=stride)                                # [B][K][P]
    return c.permute(0, 2, 1).reshape(-1, c.shape[1]).numpy()


def _seq_conv_dw(x, dy_nhwc, k, stride, shape, nchw=False, **mut):
    cols = _cols(x, k, stride, nchw)
    dy = np.asarray(dy_nhwc, np.float32).reshape(cols.shape[0], -1)
    gw = _seq_dw(cols, dy, **mut)                                    # [cin*k*k][cout]
    gb = _seq_dw(np.ones((cols.shape[0], 1)), dy, **mut)[0]
    return gw.T.reshape(shape).copy(), gb


def _seq_dx(dy_nhwc, W, mask_nhwc, stride, out_hw, drop_tap=None, swap=None, relu=True):
    """Transposed conv in f32, terms added sequentially in (kh, kw, cout) order; mask from the previous activation.
    drop_tap: a (kh, kw) left out; swap: cin whose weight row at (kh, kw) = (0, 1) is read from (1, 0); relu=False: no mask."""
    dy = np.asarray(dy_nhwc, np.float64)
    B, OH, OW, CO = dy.shape
    W = np.asarray(W, np.float64)                                    # [cout][cin][kh][kw]
    K = W.shape[2]
    acc = np.zeros((B, out_hw, out_hw, W.shape[1]), np.float32)
    for kh in range(K):
        for kw in range(K):
            if drop_tap == (kh, kw): continue
            view = acc[:, kh:kh + stride * OH:stride, kw:kw + stride * OW:stride, :]
            for co in range(CO):
                wrow = W[co, :, kh, kw].copy()
                if swap is not None and (kh, kw) == (0, 1): wrow[swap] = W[co, swap, 1, 0]
                view[...] = _acc(view, dy[..., co:co + 1] * wrow)
    return np.where(np.asarray(mask_nhwc) > 0, acc, np.float32(0)) if relu else acc


def restatement(inp: dict, only=None, mutate: Optional[dict] = None) -> dict:
    """The fourteen outputs (or those in `only`) in sequential float32.  mutate: {output name: keyword arguments of its routine}
    - the wrong kernels of the host self-test."""
    mut = mutate or {}
    want = OPS if only is None else only
    p = [np.asarray(x, np.float32) for x in inp["params"]]
    act = np.asarray(inp["act"], np.int64)
    B, A = act.shape[0], p[8].shape[0]
    g = lambda k: np.asarray(inp[k], np.float32)
    out = {}
    if "dh1" in want:
        relu = mut.get("dh1", {}).get("relu", True)
        v = (g("dq").astype(np.float64)[:, None] * p[8][act].astype(np.float64)).astype(np.float32)
        out["dh1"] = np.where(g("h1") > 0, v, np.float32(0)) if relu else v
    if "gW5" in want or "gb5" in want:
        gw, gb = np.zeros((A, 512), np.float32), np.zeros(A, np.float32)
        for a in range(A):
            r = np.flatnonzero(act == a)
            if len(r):
                gw[a] = _seq_dw(g("dq")[r][:, None], g("h1")[r], **mut.get("gW5", {}))[0]
                gb[a] = _seq_dw(g("dq")[r][:, None], np.ones((len(r), 1), np.float32), **mut.get("gb5", {}))[0, 0]
        out["gW5"], out["gb5"] = gw, gb
    if "gW4" in want or "gb4" in want:
        a3f = np.ascontiguousarray(g("a3").transpose(0, 3, 1, 2)).reshape(B, 3136)
        out["gW4"] = _seq_dw(g("dh1"), a3f, **mut.get("gW4", {}))
        out["gb4"] = _seq_dw(np.ones((B, 1)), g("dh1"), **mut.get("gb4", {}))[0]
    if "dy3" in want:
        m = mut.get("dy3", {})
        acc = np.zeros((B, 3136), np.float32)
        dh1, W4 = g("dh1").astype(np.float64), p[6].astype(np.float64)
        for j in range(512):
            if j != m.get("drop_term"): acc = _acc(acc, dh1[:, j:j + 1] * W4[j][None, :])
        v = np.ascontiguousarray(acc.reshape(B, 64, 7, 7).transpose(0, 2, 3, 1))
        out["dy3"] = np.where(g("a3") > 0, v, np.float32(0)) if m.get("relu", True) else v
    if "gW3" in want or "gb3" in want:
        out["gW3"], out["gb3"] = _seq_conv_dw(g("a2"), g("dy3"), 3, 1, (64, 64, 3, 3), **mut.get("gW3", {}))
    if "dy2" in want:
        out["dy2"] = _seq_dx(g("dy3"), p[4], g("a2"), 1, 9, **mut.get("dy2", {}))
    if "gW2" in want or "gb2" in want:
        out["gW2"], out["gb2"] = _seq_conv_dw(g("a1"), g("dy2"), 4, 2, (64, 32, 4, 4), **mut.get("gW2", {}))
    if "dy1" in want:
        out["dy1"] = _seq_dx(g("dy2"), p[2], g("a1"), 2, 20, **mut.get("dy1", {}))
    if "gW1" in want or "gb1" in want:
        m = dict(mut.get("gW1", {}))
        scale = m.pop("scale", True)
        obs = np.asarray(inp["obs"]).reshape(B, -1, 84, 84)
        gw, out["gb1"] = _seq_conv_dw(obs, g("dy1"), 8, 4, (32, obs.shape[1], 8, 8), nchw=True, **m)
        out["gW1"] = gw * INV255_F32 if scale else gw
    return {k: v for k, v in out.items() if k in want}


# ------------------------------------------------------------------------------------------------ inputs without a device
def cpu_inputs(params_flat, shapes, obs, act, dq=None, td=None, seed=0) -> dict:
    """The inputs of reference() / restatement() from a float32 evaluation of the network on the CPU (torch): the activations
    the device would probe, up to summation order.  dq: given; or from td = (next_obs, reward, term): the SmoothL1 TD step with the
    target network equal to the online one (discount 0.99, Reduction::Mean); or N(0, 1) / B."""
    o, p = 0, []
    for s in shapes:
        n = int(np.prod(s)); p.append(np.asarray(params_flat[o:o + n], np.float32).reshape(s)); o += n
    B = obs.shape[0]
    t = [torch.from_numpy(x) for x in p]
    x = torch.from_numpy(np.ascontiguousarray(obs)).reshape(B, -1, 84, 84).float() / 255
    a1 = F.conv2d(x, t[0], t[1], stride=4).relu()
    a2 = F.conv2d(a1, t[2], t[3], stride=2).relu()
    a3 = F.conv2d(a2, t[4], t[5], stride=1).relu()
    h1 = F.linear(a3.flatten(1), t[6], t[7]).relu()
    if dq is None and td is not None:
        nobs, rew, term = td
        xn = torch.from_numpy(np.ascontiguousarray(nobs)).reshape(B, -1, 84, 84).float() / 255
        hn = F.conv2d(F.conv2d(F.conv2d(xn, t[0], t[1], stride=4).relu(), t[2], t[3], stride=2).relu(), t[4], t[5], stride=1).relu()
        qn = F.linear(F.linear(hn.flatten(1), t[6], t[7]).relu(), t[8], t[9]).max(1).values
        pred = F.linear(h1, t[8], t[9]).gather(1, torch.from_numpy(np.asarray(act, np.int64))[:, None])[:, 0]
        tgt = torch.from_numpy(np.asarray(rew, np.float32)) + (1 - torch.from_numpy(np.asarray(term, np.float32))) * 0.99 * qn
        dq = ((pred - tgt).clamp(-1, 1) / B).numpy()
    if dq is None:
        dq = (np.random.default_rng(seed).standard_normal(B) / B).astype(np.float32)
    inp = dict(params=p, obs=np.asarray(obs).reshape(B, -1, 84, 84), act=np.asarray(act, np.int64), dq=np.asarray(dq, np.float32),
               a1=_nhwc(a1).contiguous().numpy(), a2=_nhwc(a2).contiguous().numpy(), a3=_nhwc(a3).contiguous().numpy(), h1=h1.numpy())
    # the chain of intermediates, each from the restatement of the kernel that produces it
    for k in ("dh1", "dy3", "dy2", "dy1"):
        inp[k] = restatement(inp, only=(k,))[k]
    return inp


# ------------------------------------------------------------------------------------------------ the test cases
# (B, A, n_stack, double_dqn): the smallest shapes that reach each edge of the backward kernels (tests/test_gpu_dqn_backward.py)
CASES = ((1, 6, 4, False), (3, 9, 1, False), (7, 4, 8, False), (40, 6, 4, False), (65, 18, 4, True), (257, 33, 4, False))


def head_bwd_actions(B: int, A: int, seed: int) -> np.ndarray:
    """Actions for k_head_bwd's row compaction: action 0 has no rows; from B = 24 on (of the test cases: B = 40, 65 and 257) action 1 has at
    least 17 (more than one batch of 16, not a multiple of 16) - below that a batch cannot hold 17 rows of one action beside rows of
    others; the other rows go round the remaining actions (a few each: ragged batches of 16), in shuffled row order."""
    act = 1 + (np.arange(B) % (A - 1))
    if B >= 24:
        act[:17] = 1
    return act[np.random.default_rng(seed).permutation(B)].astype(np.int64)


def case_batch(B: int, A: int, ns: int, seed: int):
    """oracle.torch_ref.synthetic_atari_batch with head_bwd_actions; n_stack 1: the first frame, 8: the frames of obs and next_obs."""
    from oracle import torch_ref as T
    obs, _, nobs, rew, term = T.synthetic_atari_batch(B, A, seed)
    if ns == 1:
        obs, nobs = obs[:, :1], nobs[:, :1]
    elif ns == 8:
        obs, nobs = np.concatenate([obs, nobs], 1), np.concatenate([nobs, obs], 1)
    else:
        assert ns == 4
    return np.ascontiguousarray(obs), head_bwd_actions(B, A, seed), np.ascontiguousarray(nobs), rew, term


def case_params(A: int, ns: int, seed: int):
    from oracle import torch_ref as T
    shapes = T.cnn_shapes(A, ns)
    return T.init_params(shapes, seed), shapes


def sharp_ratios(ops: dict, val: dict) -> dict:
    """max |val - ref| / (sqrt(n) u S) per output (the figure lambda is set from)."""
    return {k: check(ops[k], val[k], np.inf).sharp_ratio for k in val}


if __name__ == "__main__":   # the restatement's ratios on the test cases' inputs (CPU evaluation of the activations): sets LAMBDA
    import sys
    sys.path.insert(0, __file__.rsplit("/tests/", 1)[0])
    worst = {k: 0.0 for k in OPS}
    for (B, A, ns, _) in CASES:
        p0, shapes = case_params(A, ns, 100 + B)
        obs, act, nobs, rew, term = case_batch(B, A, ns, 200 + B)
        inp = cpu_inputs(p0, shapes, obs, act, td=(nobs, rew, term))
        r = sharp_ratios(reference(inp), restatement(inp))
        print("B=%d A=%d ns=%d " % (B, A, ns) + " ".join("%s %.3f" % kv for kv in r.items()), flush=True)
        for k in r: worst[k] = max(worst[k], r[k])
    print("largest: " + " ".join("%s %.3f" % kv for kv in worst.items()))
