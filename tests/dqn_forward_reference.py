"""Float64 reference, float32 restatement and cases of the CNN DQN step's FORWARD kernels, one layer at a time (csrc/dqn.hip forward,
act_small_forward).  Written beside tests/dqn_backward_reference.py, whose Op, check, check_all and sharp_ratios it uses.
Nothing under border_amd/ imports this file.

Every layer is a sum of products accumulated in f32.  Each is evaluated on the device's own input of that layer (Dqn.probe): a1 from the
u8 observation rows, a2 from the probed a1, a3 from the probed a2, h1 from the probed a3, q from the probed h1, with the parameters the
test set.  So one comparison shows one layer's arithmetic and nothing of the layers in front of it.

  reference(inp, split)    per output an Op: f64 result `ref`, S = sum |a_k| |b_k| + |bias| (the same operation on absolute values),
                           reduction length n = K + 1 (K products and the bias), and an absolute allowance `extra` where the output is
                           not a bare reduction (below).  ReLU is 1-Lipschitz: |relu(x) - relu(y)| <= |x - y|, so the post-ReLU outputs
                           are compared directly and no element is exempt.
  restatement(inp, split, mutate)   the same layers in float32 with SEQUENTIAL accumulation in the device's k order; sets lambda, and with
                           `mutate` is the wrong kernel of the host self-test (tests/test_dqn_forward_reference.py).
  criteria                 (a) S == 0 -> exactly 0;  (b) |err| <= n u S;  (c) |err| <= lambda sqrt(n) u S, u = 2^-24.

Layers and layouts (the device's: activations position-major [B][H][W][C]; parameters in the reference's shapes, conv weights
[cout][cin][kh][kw], l1.weight [512][3136] with the 3136 inputs channel-major (c, h, w), l2.weight [A][512])
  a1 = relu(sum x w / 255 + b1)   K = 64 n_stack.  conv1_bf16.hpp / conv1_bf16_img.hpp: pixels 0..255 are exact bf16 values, each f32
       weight is split exactly into three bf16 terms, every product is exact, the MFMA accumulates in f32 - a bare reduction of the
       UNSCALED sum acc ~ sum x w.  Both epilogues then evaluate `acc * (1.0f / 255.0f) + bias` and clamp at 0.
         c = fl(1 / 255) = (1 + d) / 255 with |d| = |255 c - 1| = INV255_REL (0.992 u; computed below from the f32 constant);
         the compiler may contract the expression into one fma (one rounding, which is the bias step the `+ 1` in n counts) or leave
         the multiply and the add apart (then fl(acc c) adds one more rounding, <= u |acc c|).
       Against sum x w / 255 + b1 the scale therefore costs at most (INV255_REL + u) |sum x w| / 255 beyond the reduction's own bound
       (to first order in u, like (b) itself):  extra = (INV255_REL + U) |sum x w| / 255.  It is 0 where every product is 0.
       Where every product of an output is 0 (an all-zero image) the epilogue gives fma(0, c, b1) = b1 in either form:
       a1 == relu(b1) to the bit; bias_only() returns those elements and their values for the tests to compare words.
  a2 = relu(conv(a1, W2, stride 2) + b2)   K = 512;   a3 = relu(conv(a2, W3) + b3)   K = 576.
       `split` (arithmetic "bf16x3_6": FwdC2B3 / FwdC3B3 / k_fwd_c23_b3): both operands are split into three bf16 terms by split3_rn and
       six of the nine partial products are kept; the three dropped ones are <= SPLIT_C |x| |w| per product (derived in
       tests/iqn_layer_reference.py): extra = SPLIT_C * sum |x| |w|.  The exact kernels ("f32_exact": FP32 MFMA) and the acting kernels
       (k_act_layer: f32 fmaf chains) take no extra.
  h1 = relu(a3 W4^T + b4)   K = 3136 (FwdL1X: eight k-slices, summed with b4 by k_head; acting: k_act_layer<0>, seven slices).
  q  = h1 W5^T + b5         K = 512 (k_head's l2: eight fmaf per lane and a butterfly; acting: the last workgroup of k_act_layer<0>).

Restated k orders: conv1 (c, kh, kw) - 16 k per MFMA step = two patch rows of one channel; conv2 / conv3 (kh, kw, c) - the position-major
activation's own order, 32 k per step; l1 position-major (hw * 64 + c), eight slices of 13 k-tiles of 32 (the last holds 7); l2 ascending.
"""
from __future__ import annotations

import os
import sys
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_backward_reference as R  # noqa: E402
from dqn_backward_reference import Op, U, check, check_all, sharp_ratios  # noqa: E402,F401
from iqn_layer_reference import SPLIT_C  # noqa: E402

INV255_F32 = R.INV255_F32
INV255_REL = abs(255.0 * float(INV255_F32) - 1.0)      # |d| of fl(1 / 255) = (1 + d) / 255
assert INV255_REL <= U

KERNEL = {"a1": "k_conv1_bf16 / k_conv1_bf16_img", "a2": "conv2 forward", "a3": "conv3 forward", "h1": "l1 forward + k_head", "q": "k_head (l2)"}
OPS = tuple(KERNEL)
# (kernel size, stride) of the conv layers; the parameter indices of every layer's weight and bias
CONV = {"a1": (8, 4), "a2": (4, 2), "a3": (3, 1)}
PARAM = {"a1": (0, 1), "a2": (2, 3), "a3": (4, 5), "h1": (6, 7), "q": (8, 9)}
INPUT = {"a2": "a1", "a3": "a2", "h1": "a3", "q": "h1"}
L1_SLICE = 13 * 32    # k per slice of FwdL1X (98 k-tiles of 32 over 8 slices: 13 each, the last 7)

# Criterion (c)'s factor per output: 4 x the largest |err| / (sqrt(n) u S) (the split extra taken off) that the sequential float32
# restatement reaches against f64 on the inputs of RESTATEMENT_CASES (activations from a CPU evaluation of the same parameters and
# batches; both arithmetics of conv2 / conv3), floored at 1.  The 4 is the project's allowance for a different summation order (MFMA
# steps, k-slices, butterflies) - it is NOT fitted to the device.  `python tests/dqn_forward_reference.py` prints the line;
# tests/test_dqn_forward_reference.py recomputes it and fails if the cases, the seeds or the restatement move away from it.
RESTATEMENT_RATIO = {"a1": 0.338, "a2": 0.263, "a3": 0.189, "h1": 0.052, "q": 0.059}
LAMBDA = {k: max(1.0, 4.0 * v) for k, v in RESTATEMENT_RATIO.items()}

_t, _nchw, _nhwc, _acc = R._t, R._nchw, R._nhwc, R._acc


# ------------------------------------------------------------------------------------------------ f64 reference
def _conv_input(inp, name):
    if name == "a1":
        obs = np.asarray(inp["obs"])
        return _t(obs.reshape(obs.shape[0], -1, 84, 84))             # NCHW, 0..255
    return _nchw(_t(inp[INPUT[name]]))


def _layer64(inp, name):
    """(pre-activation products' sum, the same on absolute values, bias) in f64, in the device's layout."""
    W, b = (_t(inp["params"][i]) for i in PARAM[name])
    if name in CONV:
        x, (_, st) = _conv_input(inp, name), CONV[name]
        y, s = _nhwc(F.conv2d(x, W, stride=st)), _nhwc(F.conv2d(x.abs(), W.abs(), stride=st))
        if name == "a1": y, s = y / 255.0, s / 255.0
    else:
        x = _t(inp[INPUT[name]])
        if name == "h1": x = _nchw(x).reshape(x.shape[0], 3136)      # l1's input: channel-major flatten
        y, s = x @ W.t(), x.abs() @ W.abs().t()
    return y.numpy(), s.numpy(), b.numpy()


def reference(inp: dict, split: bool = False, only=None) -> dict:
    """name -> Op for a1, a2, a3, h1, q (or those in `only`).  inp: params (ten arrays in reference shapes), obs u8 [B][ns][84][84] (an
    extra unit axis is accepted), a1 [B][20][20][32], a2 [B][9][9][64], a3 [B][7][7][64], h1 [B][512] - each the input of the NEXT layer.
    split: conv2 / conv3 ran on six of the nine products of split operands."""
    out = {}
    for name in (OPS if only is None else only):
        y, s, b = _layer64(inp, name)
        ref = y + b
        if name != "q": ref = np.maximum(ref, 0.0)
        extra = None
        if name == "a1": extra = (INV255_REL + U) * np.abs(y)
        elif split and name in ("a2", "a3"): extra = SPLIT_C * s
        K = np.asarray(inp["params"][PARAM[name][0]])[0].size
        out[name] = Op(name, ref, s + np.abs(b), np.broadcast_to(np.float64(K + 1), ref.shape), None, extra, KERNEL[name])
    return out


def bias_only(inp: dict):
    """(mask, values) of the a1 elements whose every product is 0 (zero pixels under every tap): there a1 is relu(b1) to the bit."""
    _, s, _ = _layer64(inp, "a1")
    b1 = np.maximum(np.asarray(inp["params"][1], np.float32), np.float32(0))
    return s == 0, np.broadcast_to(b1, s.shape)


# ------------------------------------------------------------------------------------------------ float32 restatement
def _bf16_rn(x):
    """round-to-nearest-even bf16 of f32 values, as f32 (v_cvt_pk_bf16_f32 on finite inputs)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def split3_rn(x):
    """igemm_b3.hpp split3_rn: x = t0 + t1 + t2 exactly, every term the nearest bf16 of what the terms before it left."""
    x = np.asarray(x, np.float32)
    t0 = _bf16_rn(x); r1 = x - t0
    t1 = _bf16_rn(r1); r2 = r1 - t1
    t2 = _bf16_rn(r2)
    assert (t2 == r2).all()
    return t0, t1, t2


# the six kept products (term of x, term of w) in the kernels' order within a k-step, smallest first (igemm_b3.hpp ORD9[3..8])
KEPT = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


def _seq_layer(cols, Wm, b, *, split=False, scale=None, relu=True, kept=KEPT, skip_k=(), bias_xor=False):
    """relu(scale * sum_k cols[:, k] Wm[:, k] + b) in f32, k ascending; split: per k the `kept` products of the operands' terms.
    scale: the epilogue's `acc * c + bias` as one fma.  skip_k: k indices left out."""
    cols, Wm = np.asarray(cols, np.float32), np.asarray(Wm, np.float32)
    acc = np.zeros((cols.shape[0], Wm.shape[0]), np.float32)
    skip = set(int(k) for k in skip_k)
    if split:
        xs, ws = [t.astype(np.float64) for t in split3_rn(cols)], [t.astype(np.float64) for t in split3_rn(Wm)]
    else:
        x64, w64 = cols.astype(np.float64), Wm.astype(np.float64)
    for k in range(cols.shape[1]):
        if k in skip: continue
        if split:
            for (i, j) in kept:
                acc = _acc(acc, xs[i][:, k:k + 1] * ws[j][:, k][None, :])
        else:
            acc = _acc(acc, x64[:, k:k + 1] * w64[:, k][None, :])
    b = np.asarray(b, np.float64)
    if bias_xor: b = b[np.minimum(np.arange(b.size) ^ 1, b.size - 1)]     # (an odd count's last channel keeps its own)
    v = acc.astype(np.float64) * (1.0 if scale is None else float(scale)) + b[None, :]
    v = v.astype(np.float32)
    return np.maximum(v, np.float32(0)) if relu else v


def _conv_cols(inp, name, W):
    """im2col rows [B * P][K] and the weight matrix [cout][K] in the device's k order: (c, kh, kw) for conv1, (kh, kw, c) otherwise."""
    k, st = CONV[name]
    if name == "a1":
        obs = np.asarray(inp["obs"])
        cols = R._cols(obs.reshape(obs.shape[0], -1, 84, 84), k, st, nchw=True)
    else:
        cols = R._cols(inp[INPUT[name]], k, st)
    W = np.asarray(W, np.float32)
    co, ci = W.shape[:2]
    if name == "a1":
        return cols, W.reshape(co, -1), ci
    cols = cols.reshape(-1, ci, k, k).transpose(0, 2, 3, 1).reshape(-1, k * k * ci)
    return cols, W.transpose(0, 2, 3, 1).reshape(co, -1), ci


def _k_of(name, ci, k, c, kh, kw):
    return (c * k + kh) * k + kw if name == "a1" else (kh * k + kw) * ci + c


def restatement(inp: dict, split: bool = False, only=None, mutate: Optional[dict] = None) -> dict:
    """a1, a2, a3, h1, q (or those in `only`) in sequential float32.  mutate: {output: {mistake: argument}} - the wrong kernels of the
    host self-test:
      swap_khkw=True       the weights' kh and kw exchanged                         (a1, a2, a3)
      drop_tap=(kh, kw)    that tap of every input channel left out                 (a1, a2, a3)
      drop_last_kstep=True the last 16 (a1) / 32 (a2, a3) k of the device's order left out
      bias_xor=True        channel c takes the bias of channel c ^ 1                (every layer)
      no_scale=True        the 1 / 255 omitted                                      (a1)
      row_shift=True       the last position of every image reads the patch of the row behind it (the next image's first)   (a1, a2, a3)
      kept=(...)           the split products that are kept, e.g. five of KEPT      (a2, a3 with split)
      drop_kslice=s        slice s of l1's eight k-slices left out                  (h1)
      other_w=True         the weight of inp["params_other"] instead                (every layer)"""
    mut = mutate or {}
    out = {}
    for name in (OPS if only is None else only):
        m = dict(mut.get(name, {}))
        P = inp["params_other"] if m.pop("other_w", False) else inp["params"]
        W, b = np.asarray(P[PARAM[name][0]], np.float32), np.asarray(inp["params"][PARAM[name][1]], np.float32)
        kw = dict(bias_xor=m.pop("bias_xor", False))
        if name in CONV:
            k, _ = CONV[name]
            if m.pop("swap_khkw", False): W = np.ascontiguousarray(W.transpose(0, 1, 3, 2))
            cols, Wm, ci = _conv_cols(inp, name, W)
            skip = []
            if "drop_tap" in m:
                kh, kw_ = m.pop("drop_tap")
                skip += [_k_of(name, ci, k, c, kh, kw_) for c in range(ci)]
            if m.pop("drop_last_kstep", False):
                step = 16 if name == "a1" else 32
                skip += list(range(Wm.shape[1] - step, Wm.shape[1]))
            if m.pop("row_shift", False):
                Bn = cols.shape[0] // {"a1": 400, "a2": 81, "a3": 49}[name]
                Pn = cols.shape[0] // Bn
                last = np.arange(Bn) * Pn + Pn - 1
                cols = cols.copy(); cols[last] = cols[(last + 1) % cols.shape[0]]
            scale = None
            if name == "a1" and not m.pop("no_scale", False): scale = INV255_F32
            v = _seq_layer(cols, Wm, b, split=split and name != "a1", scale=scale, skip_k=skip, kept=m.pop("kept", KEPT), **kw)
            Bn = np.asarray(inp["obs"]).shape[0]
            out[name] = v.reshape(Bn, *{"a1": (20, 20), "a2": (9, 9), "a3": (7, 7)}[name], W.shape[0])
        elif name == "h1":
            a3 = np.asarray(inp["a3"], np.float32)
            x = a3.reshape(a3.shape[0], 3136)                                                   # position-major: hw * 64 + c
            Wm = W.reshape(512, 64, 49).transpose(0, 2, 1).reshape(512, 3136)
            skip = []
            if "drop_kslice" in m:
                s = m.pop("drop_kslice")
                skip = list(range(s * L1_SLICE, min((s + 1) * L1_SLICE, 3136)))
            out[name] = _seq_layer(x, Wm, b, skip_k=skip, **kw)
        else:
            out[name] = _seq_layer(np.asarray(inp["h1"], np.float32), W, b, relu=False, **kw)
        assert not m, "unknown mutation of %s: %s" % (name, m)
    return out


# ------------------------------------------------------------------------------------------------ inputs without a device
def unflat(params_flat, shapes) -> list:
    o, p = 0, []
    for s in shapes:
        n = int(np.prod(s)); p.append(np.asarray(params_flat[o:o + n], np.float32).reshape(s)); o += n
    return p


def cpu_inputs(params: list, obs, params_other: Optional[list] = None) -> dict:
    """The inputs of reference() / restatement() from a float32 evaluation of the network on the CPU (torch): the activations the
    device would probe, up to summation order."""
    B = obs.shape[0]
    t = [torch.from_numpy(np.ascontiguousarray(x)) for x in params]
    x = torch.from_numpy(np.ascontiguousarray(obs)).reshape(B, -1, 84, 84).float() / 255
    a1 = F.conv2d(x, t[0], t[1], stride=4).relu()
    a2 = F.conv2d(a1, t[2], t[3], stride=2).relu()
    a3 = F.conv2d(a2, t[4], t[5], stride=1).relu()
    h1 = F.linear(a3.flatten(1), t[6], t[7]).relu()
    inp = dict(params=params, obs=np.asarray(obs).reshape(B, -1, 84, 84), a1=_nhwc(a1).contiguous().numpy(), a2=_nhwc(a2).contiguous().numpy(),
               a3=_nhwc(a3).contiguous().numpy(), h1=h1.numpy())
    if params_other is not None: inp["params_other"] = params_other
    return inp


# ------------------------------------------------------------------------------------------------ the test cases
CASES = R.CASES            # (B, A, n_stack, double_dqn): tests/test_gpu_dqn_forward.py says which edge of the forward kernels each reaches
# the cases the restatement's ratios are taken from: those whose sequential evaluation takes seconds on the CPU (all n_stack forms of
# conv1, the 8- and 24-action heads)
RESTATEMENT_CASES = tuple(c for c in CASES if c[0] <= 7)
# batches that hold an all-zero and an all-255 image: B -> ((row of obs, row of next_obs) that is 0, the same for 255)
EDGE_ROWS = {7: ((1, 3), (2, 4)), 40: ((5, 7), (6, 8))}


def case_params(A: int, ns: int, Bsz: int):
    """(qnet, qnet_tgt) as lists of ten arrays, different from each other, and the shapes."""
    q, shapes = R.case_params(A, ns, 100 + Bsz)
    tg, _ = R.case_params(A, ns, 500 + Bsz)
    return q, tg, shapes


def case_batch(Bsz: int, A: int, ns: int):
    """dqn_backward_reference.case_batch with the edge images of EDGE_ROWS put in."""
    obs, act, nobs, rew, term = R.case_batch(Bsz, A, ns, 200 + Bsz)
    if Bsz in EDGE_ROWS:
        (z0, z1), (f0, f1) = EDGE_ROWS[Bsz]
        obs, nobs = obs.copy(), nobs.copy()
        obs[z0], nobs[z1], obs[f0], nobs[f1] = 0, 0, 255, 255
    return obs, act, nobs, rew, term


def case_ratios(Bsz: int, A: int, ns: int) -> dict:
    """The restatement's ratios on one case: both instances of an update (qnet on obs, qnet_tgt on next_obs), conv2 / conv3 in both arithmetics."""
    q, tg, shapes = case_params(A, ns, Bsz)
    obs, _, nobs, _, _ = case_batch(Bsz, A, ns)
    worst = {k: 0.0 for k in OPS}
    for flat, x in ((q, obs), (tg, nobs)):
        inp = cpu_inputs(unflat(flat, shapes), x)
        for split, only in ((False, OPS), (True, ("a2", "a3"))):
            r = sharp_ratios(reference(inp, split, only), restatement(inp, split, only))
            for k in r: worst[k] = max(worst[k], r[k])
    return worst


def restatement_ratios() -> dict:
    worst = {k: 0.0 for k in OPS}
    for (Bsz, A, ns, _) in RESTATEMENT_CASES:
        r = case_ratios(Bsz, A, ns)
        print("B=%d A=%d ns=%d " % (Bsz, A, ns) + " ".join("%s %.3f" % kv for kv in r.items()), flush=True)
        for k in r: worst[k] = max(worst[k], r[k])
    return worst


if __name__ == "__main__":   # the restatement's ratios on RESTATEMENT_CASES: sets LAMBDA
    sys.path.insert(0, __file__.rsplit("/tests/", 1)[0])
    print("largest: " + " ".join("%s %.3f" % kv for kv in restatement_ratios().items()))
