"""Crafted optimizer states for the Adam / AdamW / amsgrad step and the soft update, with restatements, bars and mutations.

Every agent ends its update in adam_element or adam_element_amsgrad and track_element (csrc/agent_base.hpp).  Given the device's own
gradient and the state before, the state after is a pure element-wise function, and the kernels promise to compute it with separately
rounded f32 operations.  Used by tests/test_optimizer_inputs.py (CPU) and tests/test_gpu_optimizer_edges.py (GPU):

  restatements   adam_scalars (adam_scalars_for: double arithmetic, one cast to f32 per field), adam_f32 / track_f32 (numpy float32, one
                 rounding per operation, the kernels' operation order), adam_f64 / track_f64 (the same formula in float64 from the same
                 f32 scalars: the scalars are the contract, libtorch and candle both hand the kernel f32 scalars), candle_adamw_f64 (the
                 textbook form candle-nn documents, from the configuration's doubles).
  bars           adam_bars / track_bar: the distance an f32 evaluation may keep from the float64 one, from the count of f32 roundings on
                 each quantity's path (derivation beside them).
  crafting       craft_params / craft_moments / craft_targets / make_batch: the state written before the step under test.
  mutations      MUTATIONS: wrong optimizers, restated; sensitivity() measures by how many bars each one moves a compared quantity.
  case table     CASES: agent, kernel path, optimizer configuration, step number, soft-update rate, shape.

Nothing under border_amd/ imports this file.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

F32 = np.float32
U = 2.0 ** -24            # half an ulp of an f32, relative: |fl(x) - x| <= U |x| for a normal result
SUB = 2.0 ** -150         # ... and half the spacing of the subnormals, the absolute part of every rounding


# ======================================================================================================== configurations
@dataclass(frozen=True)
class Opt:
    """OptimizerConfig (opt.rs:13-28).  kind "Adam" ignores every field but lr: tch's nn::Adam::default() is fixed."""
    kind: str = "Adam"
    lr: float = 3e-3
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    wd: float = 0.0
    amsgrad: bool = False

    @property
    def adamw(self) -> bool:
        return self.kind == "AdamW"


TCH = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.0)                       # tch nn::Adam::default() / the fields' defaults
ADAM = Opt("Adam", 3e-3)                                              # plain Adam: the fixed tch defaults
ADAMW = Opt("AdamW", 1e-2, 0.8, 0.9, 1e-3, 0.1)                       # no field equals a default
ADAMW_B = Opt("AdamW", 5e-3, 0.7, 0.95, 1e-4, 0.2)                    # a second one, for a second model of the same agent
AMSGRAD = Opt("AdamW", 1e-2, 0.8, 0.9, 1e-3, 0.1, True)
CANDLE_ALPHA = Opt("AdamW", 3e-4, 0.9, 0.999, 1e-8, 0.01)             # candle-nn ParamsAdamW::default() at EntCoef's lr (sac/ent_coef.rs)


def adam_scalars(adamw: bool, lr: float, b1: float, b2: float, eps: float, wd: float, t: int) -> dict:
    """adam_scalars_for (csrc/agent_base.hpp): double arithmetic, then one cast to f32 per field"""
    if not adamw:
        b1, b2, eps, wd = TCH["b1"], TCH["b2"], TCH["eps"], TCH["wd"]
    bc1, bc2 = 1.0 - math.pow(b1, float(t)), 1.0 - math.pow(b2, float(t))
    return dict(b1=F32(b1), omb1=F32(1.0 - b1), b2=F32(b2), omb2=F32(1.0 - b2), sqrt_bc2=F32(math.sqrt(bc2)), eps=F32(eps),
                neg_step=F32(-(lr / bc1)), wd_mul=F32(1.0 - lr * wd))


def scalars_of(o: Opt, t: int, lr: Optional[float] = None) -> dict:
    return adam_scalars(o.adamw, o.lr if lr is None else lr, o.b1, o.b2, o.eps, o.wd, t)


# ======================================================================================================== restatements
SQRT_ULPS = (0, -1, 1)   # the hardware root's distance from the rounded one, in ulps (see adam_f32)


def adam_f32(p, g, m, v, vmax, s, sqrt_ulps: int = 0):
    """adam_element / adam_element_amsgrad (vmax given) in numpy float32: every operation rounds on its own, in the kernel's order.
    Returns (p', m', v', vmax' or None).
    The one operation that is not rounded to nearest on the device is the square root: the kernels call __fsqrt_rn, which this
    toolchain maps to the hardware's v_sqrt_f32 (accurate to 1 ulp) unless OCML_BASIC_ROUNDED_OPERATIONS is defined.  `sqrt_ulps`
    moves the restated root by that many ulps; a device p' must carry the bits of one of SQRT_ULPS (DESIGN.md section 16 says why the
    root stays as it is).  exp_avg, exp_avg_sq and max_exp_avg_sq do not pass through it and admit no such choice."""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        p = p * s["wd_mul"]
        mg = g * s["omb1"]
        m = m * s["b1"] + mg
        gg = s["omb2"] * g * g
        v = v * s["b2"] + gg
        if vmax is not None:
            vmax = np.maximum(np.asarray(vmax, F32), v)
        sq = np.sqrt(vmax if vmax is not None else v)
        if sqrt_ulps:
            sq = np.nextafter(sq, F32(np.inf if sqrt_ulps > 0 else -np.inf))
        denom = sq / s["sqrt_bc2"] + s["eps"]
        upd = s["neg_step"] * m / denom
        p = p + upd
    assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32
    return p, m, v, vmax


LOG_ALPHA_FORMS = [(fm, fv, u) for fm in ("", "mb", "mg") for fv in ("", "vb", "gg") for u in SQRT_ULPS]


def log_alpha_step_f32(p, g, m, v, s, form):
    """The tch SAC's entropy-coefficient step as its three kernels write it out (k_sac_select, k_sac_q_last, k_dense_small_dx_tail):
    the operations of adam_element without the decay, but NOT under `fp contract(off)`, so the compiler may fuse one product of
    `m b1 + g omb1` and one of `v b2 + (omb2 g) g` into the sum behind it.  form = (which product of exp_avg is fused: "" none, "mb",
    "mg"; which of exp_avg_sq: "", "vb", "gg"; the root's ulps).  The device's step must carry the bits of ONE form in all three of
    log_alpha, exp_avg and exp_avg_sq.  A fused multiply-add is restated through float64: the product of two f32 is exact there."""
    fm, fv, ulps = form
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    d = lambda x: np.asarray(x, np.float64)
    fma = lambda a, b, c: (d(a) * d(b) + d(c)).astype(F32)
    with np.errstate(all="ignore"):
        m1 = {"": lambda: m * s["b1"] + g * s["omb1"], "mb": lambda: fma(m, s["b1"], g * s["omb1"]), "mg": lambda: fma(g, s["omb1"], m * s["b1"])}[fm]()
        og = s["omb2"] * g
        v1 = {"": lambda: v * s["b2"] + og * g, "vb": lambda: fma(v, s["b2"], og * g), "gg": lambda: fma(og, g, v * s["b2"])}[fv]()
        sq = np.sqrt(v1)
        if ulps:
            sq = np.nextafter(sq, F32(np.inf if ulps > 0 else -np.inf))
        p1 = p + s["neg_step"] * m1 / (sq / s["sqrt_bc2"] + s["eps"])
    return p1.astype(F32), m1.astype(F32), v1.astype(F32)


def track_f32(src, dst, tau32, omt32):
    """track_element: tau * src and (1 - tau) * dst rounded on their own, then their sum"""
    src, dst = np.asarray(src, F32), np.asarray(dst, F32)
    x = F32(tau32) * src
    y = F32(omt32) * dst
    return x + y


def tau_scalars(tau: float):
    """launch_track / ReduceAdamArgs: (float)tau and (float)(1.0 - tau)"""
    return F32(tau), F32(1.0 - tau)


def _d(s):
    return {k: float(x) for k, x in s.items()}


def adam_f64(p, g, m, v, vmax, s, mut: Sequence[str] = ()):
    """the same formula in float64 from the same f32-rounded scalars.  `mut`: formula mutations (see MUTATIONS).
    Returns (p', m', v', vmax' or None) and, in a dict, the intermediates the bars need."""
    s = _d(s)
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    pw = p * s["wd_mul"]
    mg, mb = g * s["omb1"], m * s["b1"]
    m1 = mb + mg
    gg, vb = s["omb2"] * g * g, v * s["b2"]
    v1 = vb + gg
    if vmax is not None:
        vmax = np.asarray(vmax, np.float64)
        if "amsgrad_old_v" in mut:
            x1 = np.maximum(vmax, v)                   # the maximum of the OLD second moment
        elif "amsgrad_ignored" in mut:
            x1 = vmax                                  # the arena stays as it was; the denominator falls back to v'
        else:
            x1 = np.maximum(vmax, v1)
    else:
        x1 = None
    dv = v1 if (x1 is None or "amsgrad_ignored" in mut) else x1
    if "eps_in_sqrt" in mut:
        sq = np.sqrt(dv + s["eps"])
        q = sq / s["sqrt_bc2"]
        denom = q
    elif "eps_before_div" in mut:
        sq = np.sqrt(dv)
        q = (sq + s["eps"]) / s["sqrt_bc2"]
        denom = q
    else:
        sq = np.sqrt(dv)
        q = sq / s["sqrt_bc2"]
        denom = q + s["eps"]
    num = s["neg_step"] * m1
    with np.errstate(all="ignore"):
        upd = num / denom
    p1 = pw + upd
    return (p1, m1, v1, x1), dict(pw=pw, mg=mg, mb=mb, gg=gg, vb=vb, dv=dv, sq=sq, q=q, denom=denom, num=num, upd=upd)


def track_f64(src, dst, tau32, omt32):
    return float(tau32) * np.asarray(src, np.float64) + float(omt32) * np.asarray(dst, np.float64)


def candle_adamw_f64(p, g, m, v, o: Opt, t: int):
    """candle-nn's AdamW as its documentation states it, from the configuration's doubles (no f32 scalar anywhere):
    p *= 1 - lr wd;  m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2;  m_hat = m' / (1 - b1^t);  v_hat = v' / (1 - b2^t);
    p -= lr m_hat / (sqrt(v_hat) + eps).  Plain Adam is the same with tch's defaults and wd 0."""
    b1, b2, eps, wd = (o.b1, o.b2, o.eps, o.wd) if o.adamw else (TCH["b1"], TCH["b2"], TCH["eps"], TCH["wd"])
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    p = p * (1.0 - o.lr * wd)
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    m_hat, v_hat = m1 / (1.0 - b1 ** t), v1 / (1.0 - b2 ** t)
    return p - o.lr * m_hat / (np.sqrt(v_hat) + eps), m1, v1


# ======================================================================================================== bars
def adam_bars(p, g, m, v, vmax, s):
    """How far an f32 evaluation of adam_element(_amsgrad) may lie from adam_f64 on the same f32 inputs and scalars, per element.

    Every f32 operation returns fl(x) with |fl(x) - x| <= U |x| + SUB (U = 2^-24: half an ulp; SUB: half a subnormal step).  Walking the
    kernel's operations, with e(.) the bound so far and r(x) = U |x| + SUB the rounding of the operation that produces x:
      pw    = p wd_mul                 e(pw) = r(pw)                                                       [1 rounding]
      mg    = g omb1,  mb = m b1       e(m') = r(mg) + r(mb) + r(m')                                       [3]
      gg    = (omb2 g) g               e(gg) = 2 r(gg)   (two products in a row; the first one's error rides through the second)
      vb    = v b2                     e(v') = e(gg) + r(vb) + r(v')                                       [4]
      vmax' = max(vmax, v')            e(vmax') = e(v')  (max is 1-Lipschitz and rounds nothing)
      sq    = sqrt(dv)                 e(sq) = e(dv) / sq + 2 r(sq)    (the hardware root is accurate to one ulp, not to half of one: 2 r;
                                                                        |sqrt(x + d) - sqrt(x)| = |d| / (sqrt(x + d) + sqrt(x)) <= |d| / sqrt(x);
                                                                        dv = 0 only where g = 0 and v = 0 exactly, and then e(dv) = 0)
      q     = sq / sqrt_bc2            e(q) = e(sq) / sqrt_bc2 + r(q)
      denom = q + eps                  e(denom) = e(q) + r(denom)
      num   = neg_step m'              e(num) = |neg_step| e(m') + r(num)
      upd   = num / denom              e(upd) = (e(num) + |upd| e(denom)) / (denom - e(denom)) + r(upd)    (exact for a quotient of intervals)
      p'    = pw + upd                 e(p') = e(pw) + e(upd) + r(p')                                       [13 roundings on the longest path, the root's counted twice]
    The roundings of the f32 SCALARS are not in the bar (both sides use the same ones); the candle form, which rounds no scalar, still
    agrees within it: each scalar enters exactly one operation above, and a relative error U of that scalar moves that operation's
    result by no more than its own r(.) term (test_candle_form_agrees_within_the_bar).
    Returns dict(p=, m=, v=, vmax=) of float64 arrays."""
    (p1, m1, v1, x1), w = adam_f64(p, g, m, v, vmax, s)
    sd = _d(s)
    r = lambda x: U * np.abs(x) + SUB
    e_m = r(w["mg"]) + r(w["mb"]) + r(m1)
    e_v = 2 * r(w["gg"]) + r(w["vb"]) + r(v1)
    sq = w["sq"]
    with np.errstate(all="ignore"):
        e_sq = np.where(sq > 0, e_v / np.where(sq > 0, sq, 1.0), 0.0) + 2 * r(sq)
        e_q = e_sq / sd["sqrt_bc2"] + r(w["q"])
        e_den = e_q + r(w["denom"])
        e_num = abs(sd["neg_step"]) * e_m + r(w["num"])
        e_upd = (e_num + np.abs(w["upd"]) * e_den) / np.maximum(w["denom"] - e_den, 1e-300) + r(w["upd"])
    e_p = r(w["pw"]) + e_upd + r(p1)
    return dict(p=e_p, m=e_m, v=e_v, vmax=e_v)


def track_bar(src, dst, tau32, omt32):
    """tau src, (1 - tau) dst and their sum: three roundings, each half an ulp of what it produces (src is the device's own p', exact)"""
    x, y = float(tau32) * np.asarray(src, np.float64), float(omt32) * np.asarray(dst, np.float64)
    return U * (np.abs(x) + np.abs(y) + np.abs(x + y)) + 3 * SUB


# ======================================================================================================== crafting
N_DEAD = 8          # hidden units 0..7 of the first layer are dead; 0..3 carry m = 1e-9, v = 0; 4..7 carry m = v = 0
OBS_LO, OBS_HI = 1.0, 2.0   # observations are drawn from [1, 2): with all-negative incoming weights a dead unit's pre-activation is < 0


def dead_lanes(in_dim: int, u0: int):
    """(indices with m = 1e-9, indices with m = 0) of the dead units' incoming weights and biases in the flat reference layout
    (first layer: weight [u0][in_dim], then bias [u0])"""
    def idx(rows):
        w = np.concatenate([np.arange(r * in_dim, (r + 1) * in_dim) for r in rows])
        return np.concatenate([w, u0 * in_dim + np.asarray(rows)])
    return idx(range(0, N_DEAD // 2)), idx(range(N_DEAD // 2, N_DEAD))


def craft_params(rng, n: int, in_dim: int = 0, u0: int = 0, obs_cols: int = 0, hi: float = 8.0) -> np.ndarray:
    """n parameters from +-[0.5, hi], hi <= 8 (lr wd |p| is then comparable to lr; the seven-layer shape draws from the low end,
    +-[0.5, 0.75], so that seven layers of gain do not carry g^2 past the f32 range).  With a first Mlp layer (in_dim, u0 given): the dead units'
    incoming weights are all negative - observation columns from -[4, 8], the others (action columns, |a| <= 1) from -[0.5, 1] - and so
    is their bias (-[4, 8]): pre-activation <= -4 obs_cols - 4 + (in_dim - obs_cols) < 0 for observations in [1, 2)."""
    p = rng.uniform(0.5, hi, n) * rng.choice([-1.0, 1.0], n)
    if u0:
        assert u0 >= N_DEAD and n >= u0 * in_dim + u0 and 4 * obs_cols + 4 > in_dim - obs_cols
        W = p[:u0 * in_dim].reshape(u0, in_dim)
        W[:N_DEAD, :obs_cols] = -rng.uniform(4.0, 8.0, (N_DEAD, obs_cols))
        W[:N_DEAD, obs_cols:] = -rng.uniform(0.5, 1.0, (N_DEAD, in_dim - obs_cols))
        p[u0 * in_dim:u0 * in_dim + N_DEAD] = -rng.uniform(4.0, 8.0, N_DEAD)
    return p.astype(F32)


K_LIVE = 4


def thin_hidden_layers(p, in_dim: int, units: Sequence[int]) -> np.ndarray:
    """Keeps K_LIVE live units per hidden layer of an Mlp trunk (flat reference layout, `p` from craft_params) and gives every other
    unit all-negative incoming weights and bias, magnitudes unchanged: in the first layer the units behind the dead lanes and the
    live ones (observations >= 1), above it the units from K_LIVE on (their inputs are ReLU outputs, >= 0).  For the tanh-Gaussian
    actors on the wide and the deep shape: the log-std head goes through exp() before its clamp, so a pre-activation past 88 - which
    36 or 32 live inputs of magnitude 0.5 and more reach at once - is inf times a zero mask, NaN, in the reference's backward pass as
    much as here, and a NaN gradient leaves no optimizer step to check.  Four live units per layer keep the heads' inputs in range."""
    p = np.array(p, np.float32)
    o, i = 0, in_dim
    for l, u in enumerate(units):
        first = (N_DEAD if l == 0 else 0) + K_LIVE
        W = p[o:o + u * i].reshape(u, i)
        W[first:] = -np.abs(W[first:])
        b = p[o + u * i:o + u * i + u]
        b[first:] = -np.abs(b[first:])
        o, i = o + u * i + u, u
    return p


def craft_moments(rng, g, s, amsgrad: bool, dead=None):
    """exp_avg, exp_avg_sq (and max_exp_avg_sq) before the step, from (an estimate of) the step's gradient g:
      exp_avg       |g| U(0.1, 3) with the sign of g on even indices and the opposite sign on odd ones (1e-9 U(0.5, 2), random sign, where g = 0)
      exp_avg_sq    in thirds by index: 0, g^2 U(0.5, 2), 1e4 g^2
      max_exp_avg_sq  2 v' on the indices with (i // 3) even, v' / 2 on the others, v' = b2 v + (1 - b2) g^2 the new second moment
      dead lanes    dead = (a, b): m = 1e-9, v = 0 on a; m = v = 0 on b (vmax 0 on both)"""
    g = np.asarray(g, np.float64)
    n, i = g.size, np.arange(g.size)
    sign = np.where(g != 0, np.sign(g), rng.choice([-1.0, 1.0], n)) * np.where(i % 2 == 0, 1.0, -1.0)
    m = np.where(g != 0, np.abs(g) * rng.uniform(0.1, 3.0, n), 1e-9 * rng.uniform(0.5, 2.0, n)) * sign
    v = np.where(i % 3 == 0, 0.0, np.where(i % 3 == 1, g * g * rng.uniform(0.5, 2.0, n), 1e4 * g * g))
    if dead is not None:
        a, b = dead
        m[a], v[a], m[b], v[b] = 1e-9, 0.0, 0.0, 0.0
    m, v = m.astype(F32), np.minimum(v, 1e30).astype(F32)      # (1e4 g^2 stays inside the f32 range)
    vmax = None
    if amsgrad:
        v1 = float(s["b2"]) * v.astype(np.float64) + float(s["omb2"]) * g * g
        vmax = np.where((i // 3) % 2 == 0, 2.0 * v1, 0.5 * v1)
        if dead is not None:
            vmax[dead[0]] = vmax[dead[1]] = 0.0
        vmax = vmax.astype(F32)
    return m, v, vmax


def craft_targets(rng, online) -> np.ndarray:
    """online + U(0.5, 1.5): never equal to the online network"""
    return (np.asarray(online, np.float64) + rng.uniform(0.5, 1.5, np.size(online))).astype(F32)


def synthetic_gradient(rng, n: int, dead=None) -> np.ndarray:
    """a stand-in for the device's gradient on the CPU: magnitudes log-uniform over 1e-6 .. 1e3, mixed signs, one entry in eight exactly 0
    (ReLU-dead lanes), and exactly 0 on the dead lanes"""
    g = 10.0 ** rng.uniform(-6, 3, n) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 0.125] = 0.0
    if dead is not None:
        g[dead[0]] = g[dead[1]] = 0.0
    return g.astype(F32)


def make_batch(rng, B: int, obs_dim: int, act_dim: int, discrete: int = 0) -> dict:
    """observations in [1, 2) (see craft_params), actions in (-1, 1) or indices below `discrete`, N(0, 1) rewards and noise"""
    f = lambda x: x.astype(F32)
    return dict(obs=f(rng.uniform(OBS_LO, OBS_HI, (B, obs_dim))), next_obs=f(rng.uniform(OBS_LO, OBS_HI, (B, obs_dim))),
                act=rng.integers(0, discrete, B) if discrete else f(rng.uniform(-1, 1, (B, act_dim))),
                reward=f(rng.standard_normal(B)), term=(rng.random(B) < 0.125).astype(np.int8), trunc=np.zeros(B, np.int8),
                z1=f(rng.standard_normal((B, max(act_dim, 1)))), z2=f(rng.standard_normal((B, max(act_dim, 1)))))


def dead_gradient_f64(in_dim: int, units: Sequence[int], out_dim: int, params, rows, seed: int = 0) -> np.ndarray:
    """float64 forward and backward of Mlp(in_dim -> units -> out_dim) (ReLU hidden layers) on `rows` with a random output gradient:
    the gradient of the first layer's weights and bias, flat.  The layers above the first are taken from `params` as far as they
    go and drawn at random beyond (heads differ between agents; a dead unit's gradient is 0 whatever sits above it)."""
    import torch
    rng = np.random.default_rng(seed)
    dims, o, ps = [in_dim] + list(units) + [out_dim], 0, []
    for k in range(len(dims) - 1):
        for shape in ((dims[k + 1], dims[k]), (dims[k + 1],)):
            n = int(np.prod(shape))
            src = params[o:o + n] if o + n <= len(params) else rng.uniform(-1, 1, n)
            ps.append(torch.tensor(np.asarray(src, np.float64).reshape(shape), requires_grad=True))
            o += n
    x = torch.tensor(np.asarray(rows, np.float64))
    for k in range(len(dims) - 1):
        x = x @ ps[2 * k].T + ps[2 * k + 1]
        if k < len(dims) - 2:
            x = torch.relu(x)
    x.backward(torch.tensor(rng.standard_normal(tuple(x.shape))))
    return np.concatenate([ps[0].grad.numpy().reshape(-1), ps[1].grad.numpy().reshape(-1)])


# ======================================================================================================== mutations
# name -> what a wrong kernel or host would compute.  "scalars": the scalars come from a changed configuration; "formula": adam_f64's
# `mut`; "track": the soft update; "schedule": which update tracks / which counter a model reads (restated in sensitivity()).
MUTATIONS = {
    "decay_dropped":      ("scalars", lambda o, t: (Opt(o.kind, o.lr, o.b1, o.b2, o.eps, 0.0, o.amsgrad), t)),
    "decay_l2":           ("l2", None),            # g + wd p into the moments, no decay on the parameter (torch.optim.Adam's weight_decay)
    "bc1_missing":        ("scalar_edit", lambda s, o, t: dict(s, neg_step=F32(-o.lr))),
    "bc2_missing":        ("scalar_edit", lambda s, o, t: dict(s, sqrt_bc2=F32(1.0))),
    "t_minus_1":          ("scalars", lambda o, t: (o, t - 1)),
    "t_plus_1":           ("scalars", lambda o, t: (o, t + 1)),
    "default_beta1":      ("scalars", lambda o, t: (Opt(o.kind, o.lr, TCH["b1"], o.b2, o.eps, o.wd, o.amsgrad), t)),
    "default_beta2":      ("scalars", lambda o, t: (Opt(o.kind, o.lr, o.b1, TCH["b2"], o.eps, o.wd, o.amsgrad), t)),
    "default_eps":        ("scalars", lambda o, t: (Opt(o.kind, o.lr, o.b1, o.b2, TCH["eps"], o.wd, o.amsgrad), t)),
    "betas_swapped":      ("scalars", lambda o, t: (Opt(o.kind, o.lr, o.b2, o.b1, o.eps, o.wd, o.amsgrad), t)),
    "eps_before_div":     ("formula", "eps_before_div"),
    "eps_in_sqrt":        ("formula", "eps_in_sqrt"),
    "amsgrad_old_v":      ("formula", "amsgrad_old_v"),
    "amsgrad_ignored":    ("formula", "amsgrad_ignored"),
    "tau_swapped":        ("track", "swap"),
    "track_pre_step":     ("track", "pre"),
    "track_skipped":      ("track", "skip"),
    "track_every_update": ("schedule", "every"),
    "track_next_critic":  ("track", "next"),
    "cross_model_t":      ("schedule", "cross_t"),
}
ADAMW_ONLY = {"decay_dropped", "decay_l2", "default_beta1", "default_beta2", "default_eps", "betas_swapped"}   # plain Adam has nothing configured
AMSGRAD_ONLY = {"amsgrad_old_v", "amsgrad_ignored"}


def track_schedule(interval: int, updates_per_opt: Sequence[int]):
    """The opts after which the reference tracks (dqn/base.rs:182-200, iqn/base.rs, sac/base.rs): one counter tick per opt_, whatever
    n_updates_per_opt is; at `interval` the counter returns to 0 and the target is tracked once, from the parameters after that opt's
    last update.  Returns the list of booleans, one per opt."""
    out, counter = [], 0
    for _ in updates_per_opt:
        counter += 1
        hit = counter == interval
        if hit:
            counter = 0
        out.append(hit)
    return out


def sensitivity(name: str, o: Opt, t: int, tau: float, state: dict) -> float:
    """By how many bars mutation `name` moves the most sensitive compared quantity (p', m', v', vmax', target) on `state`
    = dict(p, g, m, v, vmax, tgt, tgt_next): the case's crafted inputs.  0 where the mutation does not apply to the configuration."""
    kind, arg = MUTATIONS[name]
    p, g, m, v, vmax = (state[k] for k in ("p", "g", "m", "v", "vmax"))
    s = scalars_of(o, t)
    (p1, m1, v1, x1), _ = adam_f64(p, g, m, v, vmax, s)
    bars = adam_bars(p, g, m, v, vmax, s)
    t32, o32 = tau_scalars(tau)

    def moved(got, ref, bar):
        with np.errstate(all="ignore"):
            d = np.abs(np.asarray(got, np.float64) - ref) / bar
        return float(np.nanmax(np.where(np.isfinite(d), d, np.inf)))

    def adam_moved(res):
        q1, n1, w1, y1 = res
        out = max(moved(q1, p1, bars["p"]), moved(n1, m1, bars["m"]), moved(w1, v1, bars["v"]))
        if x1 is not None:
            out = max(out, moved(y1, x1, bars["vmax"]))
        return out

    if (name in ADAMW_ONLY and not o.adamw) or (name in AMSGRAD_ONLY and vmax is None):
        return 0.0
    if kind == "scalars":
        o2, t2 = arg(o, t)
        if t2 < 1:   # "t - 1" at the first step: bc1 = bc2 = 0, the step is infinite or NaN - as far from the bar as can be
            return math.inf
        return adam_moved(adam_f64(p, g, m, v, vmax, scalars_of(o2, t2))[0])
    if kind == "l2":
        o2 = Opt(o.kind, o.lr, o.b1, o.b2, o.eps, 0.0, o.amsgrad)
        g2 = np.asarray(g, np.float64) + o.wd * np.asarray(p, np.float64)
        return adam_moved(adam_f64(p, g2, m, v, vmax, scalars_of(o2, t))[0])
    if kind == "scalar_edit":
        return adam_moved(adam_f64(p, g, m, v, vmax, arg(s, o, t))[0])
    if kind == "formula":
        return adam_moved(adam_f64(p, g, m, v, vmax, s, mut=(arg,))[0])
    tgt = state["tgt"]
    ref_t, bar_t = track_f64(p1, tgt, t32, o32), track_bar(p1, tgt, t32, o32)
    if kind == "track":
        got = {"swap": lambda: track_f64(p1, tgt, o32, t32), "pre": lambda: track_f64(p, tgt, t32, o32), "skip": lambda: np.asarray(tgt, np.float64),
               "next": lambda: track_f64(state["p_next"], tgt, t32, o32)}[arg]()
        return moved(got, ref_t, bar_t)
    if arg == "every":   # an update between intervals: the reference keeps the target's bits, the mutant tracks
        return moved(ref_t, np.asarray(tgt, np.float64), bar_t)
    if arg == "cross_t":   # another model's counter: only visible where the counters differ (here: by state["t_other"])
        t2 = state.get("t_other", t)
        return 0.0 if t2 == t else adam_moved(adam_f64(p, g, m, v, vmax, scalars_of(o, t2))[0])
    raise KeyError(name)


def crafted_state(seed: int, o: Opt, t: int, n: int = 768, in_dim: int = 8, u0: int = 16) -> dict:
    """the CPU stand-in of one case's inputs: craft_params / craft_moments / craft_targets on a synthetic gradient"""
    rng = np.random.default_rng(seed)
    dead = dead_lanes(in_dim, u0)
    g = synthetic_gradient(rng, n, dead)
    p = craft_params(rng, n, in_dim, u0, in_dim - 2)
    m, v, vmax = craft_moments(rng, g, scalars_of(o, t), o.amsgrad, dead)
    return dict(p=p, g=g, m=m, v=v, vmax=vmax, tgt=craft_targets(rng, p), p_next=craft_params(rng, n), dead=dead)


# ======================================================================================================== shapes and cases
SHAPES = {
    "small":  dict(obs=5, act=3, units=(64,)),
    "ragged": dict(obs=70, act=5, units=(100, 36)),     # nothing a multiple of the 64-padding: every layer has padding lanes, the arena slack
    "deep":   dict(obs=5, act=3, units=(32,) * 6, hi=0.75),      # seven layers: seven segments of k_dense_reduce_adam's segment search
}
BATCH = 8
TS = (1, 2, 10, 1000)
TAUS = (0.005, 0.5, 1.0, 0.0)


@dataclass(frozen=True)
class Case:
    name: str
    agent: str                 # sac | candle_sac | iql | awac | bc | dqn_mlp | dqn_cnn | iqn
    path: str                  # the kernel path's name in DESIGN.md section 16
    kernels: tuple             # the kernels of the issue's table this case runs its step through
    shape: str = "small"
    opts: dict = field(default_factory=dict, hash=False, compare=False)   # model group -> Opt
    t: int = 1
    tau: float = 0.005
    nc: int = 2
    env: tuple = ()            # ((variable, value), ...) set while the agent is built and stepped
    extra: tuple = ()          # agent-specific: (("ent", "auto"), ("actor", "Mlp2"), ("form", "fused"), ("actions", 6))
    refusal: str = ""          # the constructor must refuse with this message instead of running

    def x(self, key, default=None):
        return dict(self.extra).get(key, default)


RA = ("k_dense_reduce_adam",)
CASES = [
    # ---- SAC (border-tch-agent): k_dense_reduce_adam over the actor, then over n_critics instances with their targets; log-alpha in the select / row-block kernels
    Case("sac_rowblock_adamw_amsgrad_t1", "sac", "row-block", RA + ("log-alpha (k_sac_q_last / tail)",), "small", dict(actor=ADAMW, critic=AMSGRAD), 1, 0.005, 2, extra=(("ent", "auto"),)),
    Case("sac_nofuse_adam_t2_nc4", "sac", "BDR_NO_SAC_FUSE", RA + ("log-alpha (k_sac_select)",), "ragged", dict(actor=ADAM, critic=ADAM), 2, 0.5, 4, env=(("BDR_NO_SAC_FUSE", "1"),), extra=(("ent", "auto"),)),
    Case("sac_deep_adamw_t10_tau1", "sac", "row-block", RA, "deep", dict(actor=ADAMW_B, critic=ADAMW), 10, 1.0, 1, extra=(("ent", "fix"),)),
    Case("sac_adam_t1000_tau0", "sac", "row-block", RA + ("log-alpha (k_sac_q_last / tail)",), "small", dict(actor=ADAM, critic=AMSGRAD), 1000, 0.0, 2, extra=(("ent", "auto"),)),
    Case("sac_nc5_refused", "sac", "constructor", (), "small", dict(actor=ADAM, critic=ADAM), 1, 0.005, 5, refusal="n_critics must be in [1,4]"),
    # ---- candle SAC: Mlp2 / Mlp3 actors, Auto log-alpha with candle-nn's AdamW defaults (k_csac_alpha)
    Case("csac_mlp2_adamw_t1", "candle_sac", "Mlp2", RA + ("log-alpha (k_csac_alpha)",), "ragged", dict(actor=ADAMW, critic=ADAMW_B), 1, 0.005, 2, extra=(("ent", "auto"), ("actor", "Mlp2"))),
    Case("csac_mlp3_adam_t2_nc4", "candle_sac", "Mlp3", RA + ("log-alpha (k_csac_alpha)",), "small", dict(actor=ADAM, critic=ADAM), 2, 0.5, 4, extra=(("ent", "auto"), ("actor", "Mlp3"))),
    Case("csac_mlp2_one_layer_refused", "candle_sac", "constructor", (), "small", dict(actor=ADAMW, critic=ADAMW), 1, 0.005, 2, extra=(("ent", "fix"), ("actor", "Mlp2")),
         refusal="the reference's trunk needs at least 2 layers"),
    Case("csac_deep_adamw_t10_tau1", "candle_sac", "Mlp2", RA, "deep", dict(actor=ADAMW, critic=ADAMW), 10, 1.0, 1, extra=(("ent", "fix"), ("actor", "Mlp2"))),
    Case("csac_amsgrad_refused", "candle_sac", "constructor", (), "small", dict(actor=ADAMW, critic=AMSGRAD), 1, 0.005, 2, refusal="candle's AdamW has no amsgrad"),
    Case("csac_nc5_refused", "candle_sac", "constructor", (), "small", dict(actor=ADAMW, critic=ADAMW), 1, 0.005, 5, refusal="n_critics must be in [1,4]"),
    # ---- IQL / AWAC (DenseAgent::mlp_backward_step)
    Case("iql_adamw_three_opts_t2", "iql", "dense-agent", RA, "small", dict(actor=ADAMW, critic=ADAMW_B, value=Opt("AdamW", 2e-2, 0.6, 0.8, 1e-2, 0.05)), 2, 0.5, 2),
    Case("iql_adam_t1_nc4", "iql", "dense-agent", RA, "ragged", dict(actor=ADAM, critic=ADAM, value=ADAM), 1, 0.005, 4),
    Case("iql_deep_t10_tau0", "iql", "dense-agent", RA, "deep", dict(actor=ADAMW, critic=ADAMW, value=ADAMW_B), 10, 0.0, 1),
    Case("awac_adamw_t10_tau1", "awac", "dense-agent", RA, "small", dict(actor=ADAMW, critic=ADAMW_B), 10, 1.0, 2),
    Case("awac_adam_t1_nc4", "awac", "dense-agent", RA, "ragged", dict(actor=ADAM, critic=ADAM), 1, 0.005, 4),
    Case("awac_nc5_refused", "awac", "constructor", (), "small", dict(actor=ADAM, critic=ADAM), 1, 0.005, 5, refusal="n_critics must be in [1,4]"),
    # ---- BC: the three kernel forms end in the same reduce + Adam, without targets
    Case("bc_general_adamw_t1", "bc", "general", RA, "small", dict(policy=ADAMW), 1, extra=(("form", "general"),)),
    Case("bc_fused_adam_t2", "bc", "fused", RA, "ragged", dict(policy=ADAM), 2, extra=(("form", "fused"),)),
    Case("bc_fused_mfma_adamw_t10", "bc", "fused_mfma", RA, "deep", dict(policy=ADAMW_B), 10, extra=(("form", "fused_mfma"),)),
    Case("bc_general_adam_t1000", "bc", "general", RA, "small", dict(policy=ADAM), 1000, extra=(("form", "general"),)),
    # ---- DQN on an Mlp: one-workgroup LDS step, the global fused step, layer by layer
    Case("dqn_mlp_lds_adamw_t1", "dqn_mlp", "LDS step", ("mlp_fused.hpp LDS step",), "small", dict(q=ADAMW), 1, 0.005),
    Case("dqn_mlp_global_adamw_t2", "dqn_mlp", "BDR_NO_MLP_LDS", ("mlp_fused.hpp global step",), "small", dict(q=ADAMW), 2, 0.5, env=(("BDR_NO_MLP_LDS", "1"),)),
    Case("dqn_mlp_layers_adam_t10_tau1", "dqn_mlp", "BDR_NO_MLP_FUSED", ("k_dense_reduce_adam", "k_track"), "ragged", dict(q=ADAM), 10, 1.0, env=(("BDR_NO_MLP_FUSED", "1"),)),
    Case("dqn_mlp_tensors_adamw_t2", "dqn_mlp", "BDR_NO_MLP_FUSED + BDR_NO_SMALL_GEMM", ("k_adam", "k_track"), "ragged", dict(q=ADAMW), 2, 0.005, env=(("BDR_NO_MLP_FUSED", "1"), ("BDR_NO_SMALL_GEMM", "1"))),
    Case("dqn_mlp_layers_amsgrad_t2", "dqn_mlp", "BDR_NO_MLP_FUSED", ("k_adam_amsgrad", "k_track"), "ragged", dict(q=AMSGRAD), 2, 0.5, env=(("BDR_NO_MLP_FUSED", "1"),)),
    Case("dqn_mlp_amsgrad_default_path_t1", "dqn_mlp", "LDS step asked, amsgrad", ("k_adam_amsgrad", "k_track"), "small", dict(q=AMSGRAD), 1, 0.0),
    Case("dqn_mlp_lds_adam_t1000", "dqn_mlp", "LDS step", ("mlp_fused.hpp LDS step",), "small", dict(q=ADAM), 1000, 0.005),
    Case("dqn_mlp_deep_layers_t2", "dqn_mlp", "layer by layer (seven layers: past the one-workgroup step)", ("k_dense_reduce_adam", "k_track"), "deep", dict(q=ADAMW_B), 2, 0.005),
    # ---- Nature-CNN DQN: k_reduce_adam's scalar body on the conv segments, its vector body on FC-512 and the head
    Case("dqn_cnn_adamw_t1_a6", "dqn_cnn", "k_reduce_adam", ("k_reduce_adam vector body", "k_reduce_adam segment body", "k_track"), "small", dict(q=ADAMW), 1, 0.5, extra=(("actions", 6),)),
    Case("dqn_cnn_adam_t2_a9", "dqn_cnn", "k_reduce_adam", ("k_reduce_adam vector body", "k_reduce_adam segment body", "k_track"), "small", dict(q=ADAM), 2, 0.005, extra=(("actions", 9),)),
    # ---- IQN
    Case("iqn_adam_t1", "iqn", "plain", ("k_adam", "k_track"), "small", dict(q=ADAM), 1, 0.5),
    Case("iqn_amsgrad_t2", "iqn", "amsgrad", ("k_adam_amsgrad", "k_track"), "small", dict(q=AMSGRAD), 2, 0.005),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def model_nets(c: Case) -> dict:
    """model group -> (in_dim, units, out_dim, observation columns) of the networks whose first layer is an Mlp layer (dead lanes)"""
    sh = SHAPES[c.shape]
    od, ad, u = sh["obs"], sh["act"], tuple(sh["units"])
    if c.agent == "sac" or c.agent in ("candle_sac", "iql", "awac"):
        out = dict(actor=(od, u, 2 * ad, od), critic=(od + ad, u, 1, od))
        if c.agent == "iql":
            out["value"] = (od, u, 1, od)
        return out
    if c.agent == "bc":
        return dict(policy=(od, u, ad, od))
    if c.agent == "dqn_mlp":
        return dict(q=(od, u, N_ACTIONS, od))
    if c.agent == "iqn":
        return dict(q=(od, u, IQN_FEATURES, od))
    return {}


N_ACTIONS = 3                                    # the Mlp DQN's and IQN's action count
IQN_FEATURES, IQN_EMBED, IQN_MERGE = 32, 16, (48,)


def param_hi(c: Case) -> float:
    """The upper end of the crafted parameters' magnitudes, +-[0.5, hi] inside the +-[0.5, 8] every case draws from.  8 where the
    network stands it.  The seven-layer shape and the two SACs draw from +-[0.5, 0.75]: seven layers of gain 8 sqrt(n) carry g^2 past
    the f32 range, and a tanh-Gaussian actor whose pre-activations run into the thousands has no finite gradient to hand the
    optimizer (the first hardware run of this table: NaN in the SAC actors' gradient arenas at hi = 8) - and without a finite gradient
    there is no optimizer step to check."""
    return min(SHAPES[c.shape].get("hi", 8.0), 0.75 if c.agent in ("sac", "candle_sac") else 8.0)


def case_configs(c: Case):
    """every (model group, Opt) of the case, log-alpha's own optimizer included"""
    out = dict(c.opts)
    if c.x("ent") == "auto":
        out["log_alpha"] = CANDLE_ALPHA if c.agent == "candle_sac" else Opt("Adam", 3e-4)
    return out


# mutation -> the cases that must catch it (sensitivity >= 10 bars on the case's crafted inputs in at least one of them)
CATCHES = {
    "decay_dropped": ["sac_rowblock_adamw_amsgrad_t1", "csac_mlp2_adamw_t1", "iql_adamw_three_opts_t2", "bc_general_adamw_t1", "dqn_mlp_lds_adamw_t1", "dqn_cnn_adamw_t1_a6"],
    "decay_l2": ["sac_rowblock_adamw_amsgrad_t1", "csac_mlp2_adamw_t1", "awac_adamw_t10_tau1", "dqn_mlp_global_adamw_t2"],
    "bc1_missing": ["sac_nofuse_adam_t2_nc4", "csac_mlp2_adamw_t1", "iql_adam_t1_nc4", "bc_fused_adam_t2", "dqn_mlp_lds_adamw_t1", "iqn_adam_t1"],
    "bc2_missing": ["sac_nofuse_adam_t2_nc4", "csac_mlp2_adamw_t1", "iql_adam_t1_nc4", "bc_fused_adam_t2", "dqn_mlp_lds_adamw_t1", "iqn_adam_t1"],
    "t_minus_1": [c.name for c in CASES if not c.refusal],
    "t_plus_1": [c.name for c in CASES if not c.refusal and c.t < 1000] + ["sac_adam_t1000_tau0"],
    "default_beta1": ["sac_rowblock_adamw_amsgrad_t1", "csac_mlp2_adamw_t1", "iql_adamw_three_opts_t2", "bc_general_adamw_t1", "dqn_mlp_lds_adamw_t1"],
    "default_beta2": ["sac_rowblock_adamw_amsgrad_t1", "csac_mlp2_adamw_t1", "iql_adamw_three_opts_t2", "bc_general_adamw_t1", "dqn_mlp_lds_adamw_t1"],
    "default_eps": ["sac_rowblock_adamw_amsgrad_t1", "csac_mlp2_adamw_t1", "iql_adamw_three_opts_t2", "bc_general_adamw_t1", "dqn_mlp_lds_adamw_t1"],
    "betas_swapped": ["sac_rowblock_adamw_amsgrad_t1", "csac_mlp2_adamw_t1", "iql_adamw_three_opts_t2", "bc_general_adamw_t1", "dqn_mlp_lds_adamw_t1"],
    "eps_before_div": ["sac_nofuse_adam_t2_nc4", "csac_mlp2_adamw_t1", "bc_general_adamw_t1", "dqn_mlp_lds_adamw_t1", "iqn_adam_t1"],
    "eps_in_sqrt": ["sac_nofuse_adam_t2_nc4", "csac_mlp2_adamw_t1", "bc_general_adamw_t1", "dqn_mlp_lds_adamw_t1", "iqn_adam_t1"],
    "amsgrad_old_v": ["sac_rowblock_adamw_amsgrad_t1", "dqn_mlp_layers_amsgrad_t2", "iqn_amsgrad_t2"],
    "amsgrad_ignored": ["sac_rowblock_adamw_amsgrad_t1", "dqn_mlp_layers_amsgrad_t2", "iqn_amsgrad_t2"],
    "tau_swapped": ["sac_rowblock_adamw_amsgrad_t1", "csac_mlp2_adamw_t1", "iql_adam_t1_nc4", "awac_adam_t1_nc4", "dqn_mlp_lds_adamw_t1", "iqn_amsgrad_t2"],
    "track_pre_step": ["sac_nofuse_adam_t2_nc4", "csac_mlp3_adam_t2_nc4", "iql_adamw_three_opts_t2", "awac_adamw_t10_tau1", "dqn_mlp_global_adamw_t2", "dqn_cnn_adamw_t1_a6", "iqn_adam_t1"],
    "track_skipped": ["sac_nofuse_adam_t2_nc4", "csac_mlp3_adam_t2_nc4", "iql_adamw_three_opts_t2", "awac_adamw_t10_tau1", "dqn_mlp_global_adamw_t2", "dqn_cnn_adamw_t1_a6", "iqn_adam_t1"],
    "track_every_update": ["dqn_mlp_global_adamw_t2", "iqn_adam_t1"],     # (the interval tests run these configurations with soft_update_interval = 3)
    "track_next_critic": ["sac_nofuse_adam_t2_nc4", "csac_mlp3_adam_t2_nc4", "iql_adam_t1_nc4", "awac_adam_t1_nc4"],
    "cross_model_t": ["iql_adamw_three_opts_t2", "sac_rowblock_adamw_amsgrad_t1"],
}
