"""Float64 reference, float32 restatement and cases of the SAC step's kernels, one layer at a time (csrc/sac.hip update_rest,
csrc/sac_fused.hpp, csrc/dense.hpp, csrc/dense_chain.hpp).  Written beside tests/iqn_layer_reference.py; Op, check and check_all are
those of tests/dqn_backward_reference.py.  Nothing under border_amd/ imports this file.

Given the device's own inputs of a kernel (Sac.layer: every raw buffer of the last update in two phases, padding included; the
parameters the test set and read back) each output is either a sum of exact products accumulated in f32 (the GEMM outputs) or a few
f32 operations per row (the row-wise outputs).

  reference(inp)          name -> Op.  GEMM outputs: f64 result, S = sum |a_k| |b_k|, n = the reduction length (terms whose dy factor is
                          exactly 0 are not counted).  ReLU masks come from the probed activation (`> 0`), the selected critic from the
                          probed Q-values by the kernel's rule (strict `<`, lowest index on a tie), the clamp indicator from the probed
                          s (lo <= s <= hi).  Arrays keep the device's padded leading dimensions and the parameters are zero-padded:
                          a padding column has S == 0 and criterion (a) demands that it is exactly 0.
                          Row-wise outputs: f64 of the same formula on the probed f32 inputs of that stage, S = bound / u with the
                          bound written out below, n = 1, lambda = 1: (b) and (c) both read |err| <= bound, (a) keeps the padding at 0.
  restatement(inp, mut)   the GEMM outputs again in float32 with sequential accumulation, products formed exactly; sets RESTATEMENT_RATIO and
                          LAMBDA = max(1, 4 x ratio) per output (critics and chunks folded, kind()), and with `mut` it is the wrong kernel
                          of the host self-test.
  criteria                (a) S == 0 -> exactly 0;  (b) |err| <= n u S;  (c) |err| <= lambda sqrt(n) u S, u = 2^-24.

Row-wise bounds (first order in u; every f32 operation contributes u x |its result|, half an ulp being <= u |x|; E, T, G are the
function constants EXPF_U, TANHF_U, LOGF_U in units of u relative to the result)
  s      = expf(e):                 E u s.
  sd     = expf(clamp(s, lo, hi)):  E u sd  (the clamp of the probed s is exact).
  a      = tanhf(sd z + mean), t = sd z + mean either one fma (u |t|) or a rounded product and an add (u |sd z| + u |t|): dt = u (|sd z| +
           |t|) covers both.  tanh is evaluated at t - dt, t, t + dt in f64; the bound is the largest distance to tanh(t) plus T u |a|
           (interval form: on a saturated row 1 - a^2 at t alone would understate the slope on the near side).
  a'     (critic phase: s and sd are not stored) the same from the probed e' and mean': ds = E u s, dsd = E u sd + sd ds 1{lo<=s<=hi},
           dt = |z| dsd + u (|sd z| + |t|).
  logp   = sum_j (-0.5 ln 2pi - 0.5 z^2) - sum_j logf((1 - a^2) + eps), one wave per row, butterfly sums over A lanes.
           per lane, with w = (1 - a^2) + eps evaluated in f64 from the probed a: a^2 rounded (u a^2; absent when contracted), 1 - .
           rounded (u |1 - a^2|), + eps rounded (u w): dw = u (a^2 + |1 - a^2| + w); the log term is off by dw / w (the conditioning
           1 / ((1 - a^2) + eps)) + G u |log w|.  The normal term: u (z^2 + 0.5 z^2 + |term|) = u (1.5 z^2 + |term|).  Each butterfly of
           A terms adds at most ceil(log2 A) u sum |terms|, the final subtraction u |logp|.  No row is exempt.
  gmean  = gu = ga (1 - a^2), ga = (alpha dlogp - dq) / B, dlogp = 2a / ((1 - a^2) + eps), alpha = expf(log_alpha).  In f64 from the
           probed a, log_alpha and (unfused path) the probed dxq; on the fused path dq is the f64 GEMM of the probed c_dy[i][0] with its
           S_dq and n_dq.  dlogp: (dw / w + u) |dlogp|;  alpha dlogp: (E + 1) u more;  ga: 2 u |ga| + (rel. error of alpha dlogp) |alpha
           dlogp| / B + e_dq / B + NC u S_dq / B (the critics' terms are added one by one);  gu: u a^2 + u |1 - a^2| on the factor and u on
           the product.  Fused path: the GEMM part S_dq (1 - a^2) / B is the Op's S with n = n_dq (criteria (b) and (c) apply to it) and the
           row-wise roundings are `extra`.  Unfused path (dq is probed), or an element whose GEMM part is 0: row-wise, S = bound / u, n = 1.
  ge     = gu z sd inr s from the probed gmean (the kernel multiplies the gu it stores): four multiplies, 4 u |ge|; inr from the probed s.
  tgt    = rs r + ((1 - term) gamma) (min_i Qt_i - alpha logp'), contraction off: k = gamma or 0 exactly;  u (|al| + |nq|) + E u |al| inside
           the bracket, times k, plus u (|rs r| + |k nq| + |tgt|).
  dout   Mse: 2 (q - tgt) / B: u |d| 2 / B + u |dout|.  SmoothL1: d or sign(d), the branch from the f32 difference as the kernel forms it.
  loss   per row: Mse d^2: 3 u d^2; SmoothL1: 3 u l.  Block partial: 32-term butterfly, 5 u sum |l| + the rows' own bounds.
  sums   the block partials one by one in block order: n u S over the probed partials.

Function constants.  The ROCm installation states no maximum-ulp figure for expf, tanhf or logf (the device library ships as bitcode
without an accuracy table; no document under the installation names one), so, as for COSF_U, they are measured against f64 libm on
the SAME f32 argument over every case of tests/test_gpu_sac_layers.py (its printed "expf ... u" etc.) and the bar is twice the
measured figure rounded up to a whole u.  See FUNC_MEASURED_U / FUNC_U below.

Layouts are the device's: W [Kp][Np] k-major, bias [Np], activations [B][Np], all sizes padded to 64."""
from __future__ import annotations

import math
import os
import re
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dqn_backward_reference import Op, U, check, check_all, sharp_ratios  # noqa: E402,F401

# measured on an MI355X (largest |f(x) - f64 f(x)| / (u |f(x)|) over every case, tests/test_gpu_sac_layers.py; logf on the 44 rows of
# the logf-probe case where its own error is observable, function_errors) -> bar = ceil(2 x measured): expf 3 u, tanhf 5 u, logf 5 u
FUNC_MEASURED_U = {"expf": 1.35, "tanhf": 2.09, "logf": 2.29}
FUNC_U = {k: float(math.ceil(2.0 * v)) for k, v in FUNC_MEASURED_U.items()}
LN_SQRT_2PI = 0.91893853320467274178


def f32(x) -> float:
    """a configuration value as the kernels receive it: (float)cfg.x"""
    return float(np.float32(x))


def pad64(x: int) -> int:
    return (x + 63) // 64 * 64


def _d(x):
    return np.asarray(x, np.float64)


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    B: int
    O: int
    A: int
    pi: tuple
    q: tuple
    NC: int = 2
    ent: tuple = ("Auto", -3.0, 1e-3)
    loss: str = "Mse"
    reward_scale: float = 1.0
    env: tuple = ()                 # environment of the agent
    batches: tuple = ()             # batch sizes of the updates on one agent (default: (B,))
    special: str = ""               # "saturated": two bit-identical critics (every row ties)
    head_scale: float = 1.0         # factor on the heads' parameters: |mean| into tanh's saturation, s = exp(e) across the clamp
    seed: int = 0
    eps: float = 1e-4
    lo: float = -20.0
    hi: float = 2.0
    gamma: float = 0.99

    @property
    def fused(self) -> bool:        # Sac::fused() (csrc/sac.hip)
        return self.small and ("BDR_NO_SAC_FUSE", "1") not in self.env and self.A <= 32 and (self.O % 32) + self.A <= 32 and len(self.q) >= 1

    @property
    def small(self) -> bool:
        return ("BDR_NO_SMALL_GEMM", "1") not in self.env


CASES = {c.name: c for c in (
    Case("tiny-padded", 3, 5, 2, (64,), (64,), NC=1, ent=("Fix", 0.2), seed=1),
    Case("a17-edge", 33, 15, 17, (96, 40), (72, 136), ent=("Auto", -17.0, 1e-3), loss="SmoothL1", reward_scale=2.5, seed=2,
         gamma=0.05),   # (log p' of 17 dimensions is about -17: a small discount keeps TD residuals on both sides of the SmoothL1 kink)
    Case("a32", 40, 32, 32, (64,), (64, 64), seed=3),
    Case("unfused-a33", 65, 9, 33, (64, 64), (64, 64), seed=4),
    Case("unfused-o30", 65, 30, 8, (64, 64), (64, 64), loss="SmoothL1", seed=5),
    Case("chain", 72, 17, 6, (256, 256), (256, 256), seed=6),
    Case("chain-tpw1", 72, 17, 6, (256, 256), (256, 256), env=(("BDR_SAC_CHAIN_TPW", "1"),), seed=6),
    Case("chain-tpw4", 72, 17, 6, (256, 256), (256, 256), env=(("BDR_SAC_CHAIN_TPW", "4"),), seed=6),
    Case("chain-heads", 72, 17, 6, (256, 256), (256, 256), env=(("BDR_SAC_HEADS_FUSE", "1"),), seed=6),
    Case("chain-ragged", 72, 17, 6, (256, 40), (256, 136), NC=3, seed=7),
    Case("wide-k", 33, 7, 3, (64,), (512, 64), seed=8),
    Case("chunked-dw", 515, 11, 3, (64,), (64, 64), NC=3, batches=(515, 1290, 40), loss="SmoothL1", seed=9),
    Case("deep", 33, 23, 7, (128, 64, 32), (64, 64, 64, 64), NC=4, seed=26),   # (a seed at which more than one critic is the minimum somewhere)
    Case("big-tiles", 130, 17, 6, (64, 64), (64, 64), env=(("BDR_NO_SMALL_GEMM", "1"),), seed=11),
    Case("saturated", 64, 8, 4, (64,), (64, 64), special="saturated", head_scale=14.0, lo=0.5, hi=1.5, seed=12),   # s = exp(e) > 0: a positive min_lstd makes "below" reachable
    Case("logf-probe", 64, 3, 1, (64,), (64,), NC=1, ent=("Fix", 0.5), head_scale=8.0, seed=13),
)}


def layers(c: Case, net: str):
    """(in, out, Kp, Np, relu) per layer: pi = trunk + heads ml, sl; q = critic."""
    if net == "pi":
        d = [(i, o, 1) for i, o in zip((c.O,) + c.pi[:-1], c.pi)] + [(c.pi[-1], c.A, 0)] * 2
    else:
        d = [(i, o, 1) for i, o in zip((c.O + c.A,) + c.q, c.q)] + [(c.q[-1], 1, 0)]
    return [(i, o, pad64(i), pad64(o), r) for i, o, r in d]


def shapes(c: Case, net: str):
    return [s for (i, o, _, _, _) in layers(c, net) for s in ((o, i), (o,))]


def internal(flat, c: Case, net: str):
    """reference order (weight [out][in], bias [out] per layer) -> [(W [Kp][Np], b [Np])] zero-padded, dtype kept."""
    flat = np.asarray(flat)
    out, o = [], 0
    for (i, n, kp, np_, _) in layers(c, net):
        W = np.zeros((kp, np_), flat.dtype); b = np.zeros(np_, flat.dtype)
        W[:i, :n] = flat[o:o + n * i].reshape(n, i).T; o += n * i
        b[:n] = flat[o:o + n]; o += n
        out.append((W, b))
    return out


def arena(c: Case, net: str, raw):
    """the raw padded gradient arena -> [(gW [Kp][Np], gb [Np])]."""
    out, o = [], 0
    for (_, _, kp, np_, _) in layers(c, net):
        out.append((raw[o:o + kp * np_].reshape(kp, np_), raw[o + kp * np_:o + kp * np_ + np_])); o += kp * np_ + np_
    return out


def case_params(c: Case):
    """pi, [q_i] flat f32 in reference order, deterministic from the case's seed."""
    def init(shp, seed, scale=1.0):
        rng, out, fan = np.random.default_rng(seed), [], 1
        for s in shp:
            if len(s) > 1: fan = s[1]
            out.append((rng.uniform(-1, 1, s) * scale / math.sqrt(fan)).astype(np.float32).ravel())
        return np.concatenate(out)
    pi = init(shapes(c, "pi"), 1000 + c.seed, 0.5)
    qs = [init(shapes(c, "q"), 2000 + 10 * c.seed + i) for i in range(c.NC)]
    if c.head_scale != 1.0:
        # heads scaled up: |mean| reaches tanh's saturation (a == +-1.0f) and e spreads s = exp(e) over all three clamp states
        n_heads = 2 * (c.A * c.pi[-1] + c.A)
        pi[-n_heads:] *= np.float32(c.head_scale)
    if c.special == "saturated":
        qs = [qs[0].copy() for _ in range(c.NC)]        # bit-identical critics: every row ties
    return pi, qs


def case_batch(c: Case, B: int, step: int = 0):
    rng = np.random.default_rng(3000 + 100 * c.seed + step)
    obs = rng.standard_normal((B, c.O)).astype(np.float32)
    nobs = rng.standard_normal((B, c.O)).astype(np.float32)
    act = rng.uniform(-1, 1, (B, c.A)).astype(np.float32)
    rew = (rng.standard_normal(B) * 2).astype(np.float32)
    term = (np.arange(B) % 4 == 1).astype(np.int8)
    z1 = rng.standard_normal((B, c.A)).astype(np.float32)
    z2 = rng.standard_normal((B, c.A)).astype(np.float32)
    return obs, act, nobs, rew, term, z1, z2


def dw_rows(c: Case, B: int, chunks: int):
    """row ranges of the weight-gradient chunks: k_dense_dw_small_group (per_chunk rounded up to 32) / igemm_red_body (32-row tiles)."""
    if c.small:
        per = ((B + chunks - 1) // chunks + 31) // 32 * 32
    else:
        n_mt = (B + 31) // 32
        per = (n_mt + chunks - 1) // chunks * 32
    return [(k * per, min(B, (k + 1) * per)) for k in range(chunks)]


# ------------------------------------------------------------------------------------------------ the step on the host (inputs without a device)
def select(q):
    """k_sac_select / k_sac_q_last: index of the minimum over critics, strict `<`, lowest index on a tie.  q [NC][B]."""
    im = np.zeros(q.shape[1], np.int64); qm = q[0].copy()
    for i in range(1, q.shape[0]):
        lt = q[i] < qm
        im[lt] = i; qm = np.where(lt, q[i], qm)
    return im, qm


def simulate(c: Case, pi_flat, q_flats, qt_flats, batch, log_alpha, dtype=np.float32, chunks=None, pi1_flat=None):
    """Every buffer Sac.layer returns, computed on the host in `dtype` (float32: what the device would hold up to summation order;
    float64: the exact chain, for the comparison with autograd).  Layouts padded as on the device.  pi1_flat: the actor after its
    step (default: unchanged - the host tests do not model Adam).  Returns the `inp` of reference()."""
    obs, act, nobs, rew, term, z1, z2 = batch
    B, O, A, NC = obs.shape[0], c.O, c.A, c.NC
    f = lambda x: np.asarray(x, dtype)
    Lp, Lq = layers(c, "pi"), layers(c, "q")
    nt, L = len(c.pi), len(Lq)
    P0, Q, QT = internal(f(pi_flat), c, "pi"), [internal(f(x), c, "q") for x in q_flats], [internal(f(x), c, "q") for x in qt_flats]
    P1 = internal(f(pi_flat if pi1_flat is None else pi1_flat), c, "pi")
    Ap, Kq = Lp[nt][3], Lq[0][2]

    def packed(x, K):
        o = np.zeros((B, K), dtype); o[:, :x.shape[1]] = x; return o
    relu = lambda x: np.maximum(x, 0)
    # products summed in f64 and rounded once: the same values on every host, whatever order its BLAS adds in
    mm = lambda a_, b_: (np.asarray(a_, np.float64) @ np.asarray(b_, np.float64)).astype(dtype)
    expf = (lambda x: np.exp(x.astype(np.float64)).astype(dtype))
    inp = dict(case=c, B=B, pi0=P0, pi1=P1, q=Q, qt=QT, reward=f(rew), term=np.asarray(term), log_alpha0=f([log_alpha]))
    Aph, Cph = {}, {}
    inp["actor"], inp["critic"] = Aph, Cph
    z = np.stack([f(z1), f(z2)])

    def actor_pass(ph, P, x, zz, xq, save):
        h = x
        ph["t_act"] = []
        for l in range(nt):
            h = relu(mm(h, P[l][0]) + P[l][1]); ph["t_act"].append(h)
        mean, e = mm(h, P[nt][0]) + P[nt][1], mm(h, P[nt + 1][0]) + P[nt + 1][1]
        s = expf(e[:, :A]); sd = expf(np.clip(s, dtype(f32(c.lo)), dtype(f32(c.hi))))
        a = np.tanh((sd * zz + mean[:, :A]).astype(np.float64)).astype(dtype)
        xq[:, O:O + A] = a
        w = (1 - a.astype(np.float64) ** 2) + f32(c.eps)
        ph["logp"] = ((-LN_SQRT_2PI - 0.5 * zz.astype(np.float64) ** 2).sum(1) - np.log(w).sum(1)).astype(dtype)
        ph["mean"], ph["e"] = mean, e
        if save:
            for k, v in (("a_s", a), ("s_s", s), ("sd_s", sd)):
                ph[k] = packed(v, Ap)

    def critic_pass(Pq, x):
        acts, h = [], x
        for l in range(L):
            h = mm(h, Pq[l][0]) + Pq[l][1]
            if Lq[l][4]: h = relu(h)
            acts.append(h)
        return acts

    # ---- actor phase
    Aph["x_o"], Aph["z"] = packed(f(obs), Lp[0][2]), z
    xq_a = packed(f(obs), Kq); xq_c = packed(np.concatenate([f(obs), f(act)], 1), Kq)
    actor_pass(Aph, P0, Aph["x_o"], z[0], xq_a, True)
    Aph["xq_a"], Aph["xq_c"] = xq_a, xq_c
    Aph["c_act"] = [critic_pass(Q[i], xq_a) for i in range(NC)]
    Aph["c2_act"] = [critic_pass(Q[i], xq_c) for i in range(NC)]
    qa = np.stack([Aph["c_act"][i][L - 1][:, 0] for i in range(NC)])
    im, qm = select(qa)
    la = f([log_alpha])
    if c.ent[0] == "Auto":   # EntCoef::update, first step of nn::Adam::default() at lr = ent[2]
        g = -(np.float64(Aph["logp"].astype(np.float64).mean()) + c.ent[1])
        la = f([log_alpha - c.ent[2] * g / (abs(g) + 1e-8)])
    Aph["log_alpha"] = la
    alpha = np.exp(np.float64(la[0]))
    Aph["c_dy"], Aph["dxq"] = [], []
    for i in range(NC):
        dy = [None] * L
        d = np.zeros((B, Lq[L - 1][3]), dtype); d[:, 0] = (im == i)
        dy[L - 1] = d
        for l in range(L - 2, -1, -1):
            dy[l] = mm(dy[l + 1], Q[i][l + 1][0].T) * (Aph["c_act"][i][l] > 0)
        Aph["c_dy"].append(dy)
        Aph["dxq"].append(mm(dy[0], Q[i][0][0].T))
    dq = sum(Aph["dxq"][i][:, O:O + A] for i in range(NC))
    a, s, sd = (Aph[k][:, :A].astype(np.float64) for k in ("a_s", "s_s", "sd_s"))
    gu = ((alpha * 2 * a / ((1 - a * a) + f32(c.eps)) - dq) / B) * (1 - a * a)
    inr = (s >= f32(c.lo)) & (s <= f32(c.hi))
    Aph["gmean"], Aph["ge"] = packed(gu.astype(dtype), Ap), packed((gu * z[0] * sd * inr * s).astype(dtype), Ap)
    tdy = [None] * nt
    tdy[nt - 1] = (mm(Aph["gmean"], P0[nt][0].T) + mm(Aph["ge"], P0[nt + 1][0].T)) * (Aph["t_act"][nt - 1] > 0)
    for l in range(nt - 2, -1, -1):
        tdy[l] = mm(tdy[l + 1], P0[l + 1][0].T) * (Aph["t_act"][l] > 0)
    Aph["t_dy"] = tdy
    # ---- critic phase
    Cph["x_no"] = packed(f(nobs), Lp[0][2]); Cph["z"] = z
    xq_n = packed(f(nobs), Kq)
    actor_pass(Cph, P1, Cph["x_no"], z[1], xq_n, False)
    Cph["xq_n"], Cph["xq_c"] = xq_n, xq_c
    Cph["c_act"] = [critic_pass(QT[i], xq_n) for i in range(NC)]
    Cph["c2_act"] = Aph["c2_act"]
    qt = np.stack([Cph["c_act"][i][L - 1][:, 0] for i in range(NC)]).astype(np.float64)
    k = (1.0 - np.asarray(term, np.float64)) * f32(c.gamma)
    tgt = (f32(c.reward_scale) * rew.astype(np.float64) + k * (qt.min(0) - alpha * Cph["logp"].astype(np.float64))).astype(dtype)
    Cph["tgt"], Cph["log_alpha"] = tgt, la
    Cph["c_dy"] = []
    loss_rows = []
    for i in range(NC):
        d = (Aph["c2_act"][i][L - 1][:, 0] - tgt).astype(dtype)
        if c.loss == "SmoothL1":
            zz = np.abs(d); lr = np.where(zz < 1, 0.5 * zz * zz, zz - 0.5); g = np.where(zz < 1, d, np.sign(d))
        else:
            lr, g = d * d, 2 * d
        loss_rows.append(lr)
        dy = [None] * L
        dd = np.zeros((B, Lq[L - 1][3]), dtype); dd[:, 0] = g / dtype(B)
        dy[L - 1] = dd
        for l in range(L - 2, -1, -1):
            dy[l] = mm(dy[l + 1], Q[i][l + 1][0].T) * (Aph["c2_act"][i][l] > 0)
        Cph["c_dy"].append(dy)
    # ---- batch-wide sums: block partials [3 + NC][nb]
    nb = (B + 31) // 32
    rows = [Aph["logp"].astype(np.float64) + (c.ent[1] if c.ent[0] == "Auto" else 0.0), Aph["logp"].astype(np.float64), qm.astype(np.float64)] + \
           [x.astype(np.float64) for x in loss_rows]
    lrow = np.zeros((3 + NC, nb), dtype)
    for r, v in enumerate(rows):
        vv = np.zeros(nb * 32); vv[:B] = v
        lrow[r] = vv.reshape(nb, 32).sum(1)
    Cph["lrow"] = lrow
    scal = np.zeros(4, dtype)
    scal[1] = (alpha * lrow[1].astype(np.float64).sum() - lrow[2].astype(np.float64).sum()) / B
    scal[0] = sum(lrow[3 + i].astype(np.float64).sum() / (B * NC) for i in range(NC))
    Cph["scal"] = scal
    # ---- weight gradients: partials per chunk, then the arena
    nch = chunks if chunks is not None else 1
    inp["pi_chunks"], inp["q_chunks"] = [nch] * (nt + 2), [nch] * L

    def dws(xs, dys, lay):
        parts, ar = [], []
        for l, (x, dy) in enumerate(zip(xs, dys)):
            p = np.stack([np.concatenate([mm(x[r0:r1].T, dy[r0:r1]).ravel(), dy[r0:r1].sum(0)]) for r0, r1 in dw_rows(c, B, nch)]).astype(dtype)
            parts.append(p); ar.append(p.astype(np.float64).sum(0).astype(dtype))
        return parts, np.concatenate(ar)
    hin = Aph["t_act"][nt - 1]
    Cph["pi_part"], Cph["pi_grad"] = dws([Aph["x_o"]] + Aph["t_act"][:nt - 1] + [hin, hin], tdy + [Aph["gmean"], Aph["ge"]], Lp)
    Cph["q_part"], Cph["q_grad"] = [], []
    for i in range(NC):
        p, g = dws([xq_c] + Aph["c2_act"][i][:L - 1], Cph["c_dy"][i], Lq)
        Cph["q_part"].append(p); Cph["q_grad"].append(g)
    return inp


# ------------------------------------------------------------------------------------------------ GEMM operations
def _count(dy, axis):
    return np.maximum((np.asarray(dy) != 0).sum(axis), 1).astype(np.float64)


def _op(name, kern, ref, S, n, extra=None):
    ref = np.asarray(ref, np.float64)
    return Op(name, ref, np.broadcast_to(np.asarray(S, np.float64), ref.shape), np.broadcast_to(np.asarray(n, np.float64), ref.shape), None,
              None if extra is None else np.broadcast_to(np.asarray(extra, np.float64), ref.shape), kern)


def _fwd(x, Wb, n_in, relu):
    x, W, b = _d(x), _d(Wb[0]), _d(Wb[1])
    ref, S = x @ W + b, np.abs(x) @ np.abs(W) + np.abs(b)
    return (np.maximum(ref, 0) if relu else ref), S, n_in + 1


def _dx(dy, W, mask):
    dyd, W = _d(dy), _d(W)
    ref, S = dyd @ W.T, np.abs(dyd) @ np.abs(W).T
    if mask is not None:
        m = np.asarray(mask) > 0
        ref, S = ref * m, S * m
    return ref, S, _count(dy, 1)[:, None]


def _dw(x, dy, r0, r1):
    x, dyd = _d(x)[r0:r1], _d(dy)[r0:r1]
    n = _count(dy[r0:r1], 0)
    gw, Sw = x.T @ dyd, np.abs(x).T @ np.abs(dyd)
    return (np.concatenate([gw.ravel(), dyd.sum(0)]), np.concatenate([Sw.ravel(), np.abs(dyd).sum(0)]),
            np.concatenate([np.broadcast_to(n[None, :], gw.shape).ravel(), n]))


K_FWD = "k_dense_small<false> | k_dense_chain2 | k_igemm"
K_HEADS = "k_sac_heads_action | k_sac_pi_chain_heads | dense_forward"
K_DX = "k_dense_small<true> | last_layer_dx_store"
K_DW = "k_dense_dw_small_group | k_igemm_red_group"
K_RED = "k_dense_reduce_adam"


def _rowwise(name, kern, ref, bound):
    return _op(name, kern, ref, _d(bound) / U, 1.0)


def tanh_bound(t, dt, a):
    t, dt = _d(t), _d(dt)
    r = np.tanh(t)
    return np.maximum(np.abs(np.tanh(t + dt) - r), np.abs(np.tanh(t - dt) - r)) + FUNC_U["tanhf"] * U * np.abs(r) + 0 * _d(a)


def logp_op(name, a, z, eps, A):
    """log p of the rows from the probed actions a [B][>=A] and noise z [B][A]."""
    a, z = _d(a)[:, :A], _d(z)
    om = 1 - a * a
    w = om + eps
    dw = U * (a * a + np.abs(om) + w)
    lt = np.log(w)
    nt = -LN_SQRT_2PI - 0.5 * z * z
    depth = math.ceil(math.log2(A)) if A > 1 else 0
    ref = nt.sum(1) - lt.sum(1)
    bound = (dw / w + FUNC_U["logf"] * U * np.abs(lt)).sum(1) + U * (1.5 * z * z + np.abs(nt)).sum(1) \
        + depth * U * (np.abs(nt).sum(1) + np.abs(lt).sum(1)) + U * np.abs(ref)
    return _rowwise(name, "k_sac_heads_action | k_sac_action", ref, bound)


def action_ops(pre, ph, c: Case, z, stored: bool, xq, kern="k_sac_heads_action | k_sac_action"):
    """s, sd, a (actor phase: from the stored stages) or a' alone (critic phase: from e' and mean')."""
    A, O = c.A, c.O
    E, out = FUNC_U["expf"] * U, {}
    e, mean, z = _d(ph["e"])[:, :A], _d(ph["mean"])[:, :A], _d(z)
    if stored:
        Ap = ph["s_s"].shape[1]
        padz = lambda v: np.concatenate([v, np.zeros((v.shape[0], Ap - A))], 1)
        s_ref = np.exp(e)
        out[pre + "s"] = _rowwise(pre + "s", kern, padz(s_ref), padz(E * s_ref))
        s = _d(ph["s_s"])[:, :A]
        sd_ref = np.exp(np.clip(s, f32(c.lo), f32(c.hi)))
        out[pre + "sd"] = _rowwise(pre + "sd", kern, padz(sd_ref), padz(E * sd_ref))
        sd = _d(ph["sd_s"])[:, :A]
        t = sd * z + mean
        dt = U * (np.abs(sd * z) + np.abs(t))
        a_ref = np.tanh(t)
        out[pre + "a"] = _rowwise(pre + "a", kern, padz(a_ref), padz(tanh_bound(t, dt, a_ref)))
    else:
        s = np.exp(e); cl = np.clip(s, f32(c.lo), f32(c.hi)); sd = np.exp(cl)
        ds = E * s
        dsd = E * sd + sd * ds * ((s >= f32(c.lo)) & (s <= f32(c.hi)))
        t = sd * z + mean
        dt = np.abs(z) * dsd + U * (np.abs(sd * z) + np.abs(t))
        a_ref = np.tanh(t)
        out[pre + "a"] = _rowwise(pre + "a", kern, a_ref, tanh_bound(t, dt, a_ref))
    return out


def reference(inp: dict) -> dict:
    """name -> Op for every output of one update.  `device(inp)` gives the matching device values."""
    c, B = inp["case"], inp["B"]
    Aph, Cph = inp["actor"], inp["critic"]
    Lp, Lq = layers(c, "pi"), layers(c, "q")
    nt, L, NC, A, O = len(c.pi), len(Lq), c.NC, c.A, c.O
    ops = {}

    def put(name, kern, t):
        ops[name] = _op(name, kern, *t)

    # ---------------- actor phase
    for tag, ph, P, x in (("pi", Aph, inp["pi0"], Aph["x_o"]), ("pi'", Cph, inp["pi1"], Cph["x_no"])):
        h = x
        for l in range(nt):
            put("%s.h%d" % (tag, l), K_FWD, _fwd(h, P[l], Lp[l][0], True)); h = ph["t_act"][l]
        put(tag + ".mean", K_HEADS, _fwd(h, P[nt], Lp[nt][0], False))
        put(tag + ".e", K_HEADS, _fwd(h, P[nt + 1], Lp[nt][0], False))
    ops.update(action_ops("pi.", Aph, c, Aph["z"][0], True, Aph["xq_a"]))
    ops.update(action_ops("pi'.", Cph, c, Cph["z"][1], False, Cph["xq_n"]))
    ops["pi.logp"] = logp_op("pi.logp", Aph["a_s"], Aph["z"][0], f32(c.eps), A)
    ops["pi'.logp"] = logp_op("pi'.logp", Cph["xq_n"][:, O:O + A], Cph["z"][1], f32(c.eps), A)
    for tag, ph, key, Ps, x in (("a", Aph, "c_act", inp["q"], Aph["xq_a"]), ("c", Aph, "c2_act", inp["q"], Aph["xq_c"]), ("t", Cph, "c_act", inp["qt"], Cph["xq_n"])):
        for i in range(NC):
            h = x
            for l in range(L):
                kern = K_FWD if l < L - 1 or not c.fused else ("k_sac_td_last" if tag == "t" else "k_sac_q_last")
                put("q%d.%s.h%d" % (i, tag, l), kern, _fwd(h, Ps[i][l], Lq[l][0], bool(Lq[l][4]))); h = ph[key][i][l]
    qa = np.stack([np.asarray(Aph["c_act"][i][L - 1])[:, 0] for i in range(NC)])
    im, qm = select(qa)
    alpha = np.exp(_d(Aph["log_alpha"])[0])
    e_alpha = FUNC_U["expf"] * U * alpha
    dq, S_dq, n_dq = 0.0, 0.0, 0.0
    for i in range(NC):
        d = np.zeros(Aph["c_dy"][i][L - 1].shape); d[:, 0] = (im == i)
        ops["q%d.a.dy%d" % (i, L - 1)] = _op("q%d.a.dy%d" % (i, L - 1), "k_sac_q_last | k_sac_select", d, d, 1.0)
        for l in range(L - 2, -1, -1):
            put("q%d.a.dy%d" % (i, l), K_DX, _dx(Aph["c_dy"][i][l + 1], inp["q"][i][l + 1][0], Aph["c_act"][i][l]))
        r, S, n = _dx(Aph["c_dy"][i][0], inp["q"][i][0][0], None)
        if not c.fused:
            put("q%d.a.dxq" % i, "k_dense_small<true>", (r, S, n))
            r, S, n = _d(Aph["dxq"][i]), np.abs(_d(Aph["dxq"][i])) , np.ones((B, 1))   # the probed values enter the sum over critics
        dq, S_dq, n_dq = dq + r[:, O:O + A], S_dq + S[:, O:O + A], n_dq + np.broadcast_to(n, r.shape)[:, O:O + A]
    # tanh-Gaussian backward
    Ap = Aph["a_s"].shape[1]
    padz = lambda v: np.concatenate([v, np.zeros((B, Ap - A))], 1)
    a, s, sd, z = _d(Aph["a_s"])[:, :A], _d(Aph["s_s"])[:, :A], _d(Aph["sd_s"])[:, :A], _d(Aph["z"][0])
    om = 1 - a * a; w = om + f32(c.eps)
    dlogp = 2 * a / w
    r_dl = U * (a * a + np.abs(om) + w) / w + U
    ad = alpha * dlogp
    r_ad = r_dl + (FUNC_U["expf"] + 1) * U
    ga = (ad - dq) / B
    # the critics' terms are added one by one on either path (dq += ...): NC roundings of at most u S_dq each
    e_ga = 2 * U * np.abs(ga) + r_ad * np.abs(ad) / B + (NC * U * S_dq) / B
    gu = ga * om
    e_gu = np.abs(om) * e_ga + np.abs(ga) * U * (a * a + np.abs(om)) + U * np.abs(gu)
    S_g = (S_dq * np.abs(om) / B) if c.fused else np.zeros_like(gu)
    k_bwd = "k_sac_actor_bwd" if c.fused else "k_sac_actor_grad"
    # fused path, where the GEMM part is there: S and n are the GEMM's, the row-wise roundings are `extra`.  Elsewhere (the unfused
    # path, whose dq is probed; an element whose S_g is 0) the element is row-wise: S = bound / u, n = 1 - nothing on top of the bound.
    gem = S_g > 0
    ops["pi.gmean"] = _op("pi.gmean", k_bwd, padz(gu), padz(np.where(gem, S_g, e_gu / U)), np.maximum(padz(np.where(gem, n_dq * np.ones_like(gu), 1.0)), 1.0),
                          padz(np.where(gem, e_gu, 0.0)))
    inr = ((s >= f32(c.lo)) & (s <= f32(c.hi))).astype(np.float64)
    gmean_dev = _d(Aph["gmean"])[:, :A]
    ge = gmean_dev * z * sd * inr * s     # from the probed gmean: the kernel multiplies the value it stores
    ops["pi.ge"] = _rowwise("pi.ge", k_bwd, padz(ge), padz(4 * U * np.abs(ge)))
    # heads' input gradient and the trunk
    P0 = inp["pi0"]
    gm, gs = _d(Aph["gmean"]), _d(Aph["ge"])
    m = np.asarray(Aph["t_act"][nt - 1]) > 0
    ref = (gm @ _d(P0[nt][0]).T + gs @ _d(P0[nt + 1][0]).T) * m
    S = (np.abs(gm) @ np.abs(_d(P0[nt][0])).T + np.abs(gs) @ np.abs(_d(P0[nt + 1][0])).T) * m
    ops["pi.dy%d" % (nt - 1)] = _op("pi.dy%d" % (nt - 1), "k_sac_actor_bwd | dense_dx (accum)", ref, S, (_count(Aph["gmean"], 1) + _count(Aph["ge"], 1) + 1)[:, None])
    for l in range(nt - 2, -1, -1):
        put("pi.dy%d" % l, K_DX, _dx(Aph["t_dy"][l + 1], P0[l + 1][0], Aph["t_act"][l]))
    # ---------------- critic phase: target, losses, gradients
    qt = np.stack([_d(Cph["c_act"][i][L - 1])[:, 0] for i in range(NC)])
    qmin = qt.min(0)
    lp2, rew, term = _d(Cph["logp"]), _d(inp["reward"]), _d(inp["term"])
    al = alpha * lp2; nq = qmin - al
    k = (1 - term) * f32(c.gamma)
    rs = f32(c.reward_scale)
    tgt = rs * rew + k * nq
    e_t = np.abs(k) * (U * (np.abs(al) + np.abs(nq)) + (FUNC_U["expf"] * U) * np.abs(al)) + U * (np.abs(rs * rew) + np.abs(k * nq) + np.abs(tgt))
    ops["tgt"] = _rowwise("tgt", "k_sac_td_last | k_sac_critic_td", tgt, e_t)
    tg = np.asarray(Cph["tgt"], np.float32)
    loss_rows, e_rows = [], []
    for i in range(NC):
        q = np.asarray(Aph["c2_act"][i][L - 1], np.float32)[:, 0]
        d32 = (q - tg).astype(np.float32)                # the branch the kernel takes: from its own f32 difference
        d = _d(Aph["c2_act"][i][L - 1])[:, 0] - _d(Cph["tgt"])   # (the probed f32 values, exactly; an f64 chain of the host test keeps its own)
        if c.loss == "SmoothL1":
            zz = np.abs(d); small = np.abs(d32) < 1
            lr = np.where(small, 0.5 * zz * zz, zz - 0.5); g = np.where(small, d, np.sign(d32))
            e_g = np.where(small, U * np.abs(d), 0.0)
        else:
            lr, g, e_g = d * d, 2 * d, 2 * U * np.abs(d)
        dv = np.zeros(Cph["c_dy"][i][L - 1].shape); dv[:, 0] = g / B
        eb = np.zeros(dv.shape); eb[:, 0] = e_g / B + U * np.abs(g / B)
        ops["q%d.c.dy%d" % (i, L - 1)] = _rowwise("q%d.c.dy%d" % (i, L - 1), "k_sac_td_last | k_sac_critic_td", dv, eb)
        loss_rows.append(lr); e_rows.append(3 * U * np.abs(lr) + U * np.abs(d))
        for l in range(L - 2, -1, -1):
            put("q%d.c.dy%d" % (i, l), K_DX, _dx(Cph["c_dy"][i][l + 1], inp["q"][i][l + 1][0], Aph["c2_act"][i][l]))
    # ---------------- batch-wide sums (fused path: block partials in lrow; the scalars from the probed partials)
    nb = (B + 31) // 32
    lp1 = _d(Aph["logp"])
    tgt_e = c.ent[1] if c.ent[0] == "Auto" else 0.0
    tgt_e = np.float64(np.float32(tgt_e))

    def blocks(v, e):
        vv, ee = np.zeros(nb * 32), np.zeros(nb * 32); vv[:B] = v; ee[:B] = np.abs(v) * 5 * U + e
        return vv.reshape(nb, 32).sum(1), ee.reshape(nb, 32).sum(1)
    if c.fused:
        rows = [blocks(lp1 + tgt_e, U * np.abs(lp1 + tgt_e)), blocks(lp1, 0.0), blocks(qm.astype(np.float64), 0.0)] + [blocks(l, e) for l, e in zip(loss_rows, e_rows)]
        ops["lrow"] = _rowwise("lrow", "k_sac_q_last | k_sac_td_last", np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
        lr = _d(Cph["lrow"])
        s_lp, s_qm = lr[1].sum(), lr[2].sum()
        e_lp, e_qm = nb * U * np.abs(lr[1]).sum(), nb * U * np.abs(lr[2]).sum()
        s_l = [lr[3 + i].sum() for i in range(NC)]; e_l = [nb * U * np.abs(lr[3 + i]).sum() for i in range(NC)]
    else:   # one workgroup: the same tree from the probed rows (k_sac_select / k_sac_critic_td)
        bl = [blocks(lp1, 0.0), blocks(qm.astype(np.float64), 0.0)] + [blocks(l, e) for l, e in zip(loss_rows, e_rows)]
        tot = [(b[0].sum(), b[1].sum() + nb * U * np.abs(b[0]).sum()) for b in bl]
        (s_lp, e_lp), (s_qm, e_qm) = tot[0], tot[1]
        s_l, e_l = [t[0] for t in tot[2:]], [t[1] for t in tot[2:]]
    la_ref = alpha * s_lp - s_qm
    ops["loss_actor"] = _rowwise("loss_actor", "actor_loss_sum", [la_ref / B],
                                 [(alpha * e_lp + e_qm + (FUNC_U["expf"] + 1) * U * np.abs(alpha * s_lp) + U * np.abs(la_ref)) / B + 2 * U * np.abs(la_ref) / B])
    scale = 1.0 / (B * NC)
    lc = sum(s * scale for s in s_l)
    ops["loss_critic"] = _rowwise("loss_critic", "add_scaled", [lc], [sum(e * scale for e in e_l) + (2 * NC + 2) * U * sum(abs(s) * scale for s in s_l)])
    # ---------------- weight gradients: every chunk's partial, then the reduce's sum
    hin = Aph["t_act"][nt - 1]
    jobs = [("pi", l, x, dy, inp["pi_chunks"][l]) for l, (x, dy) in enumerate(zip([Aph["x_o"]] + list(Aph["t_act"][:nt - 1]) + [hin, hin], list(Aph["t_dy"]) + [Aph["gmean"], Aph["ge"]]))]
    for i in range(NC):
        jobs += [("q%d" % i, l, x, dy, inp["q_chunks"][l]) for l, (x, dy) in enumerate(zip([Cph["xq_c"]] + list(Aph["c2_act"][i][:L - 1]), Cph["c_dy"][i]))]
    for net, l, x, dy, nch in jobs:
        for k_, (r0, r1) in enumerate(dw_rows(c, B, nch)):
            put("%s.dW%d.part%d" % (net, l, k_), K_DW, _dw(x, dy, r0, r1))
        part = _d(Cph["pi_part"][l] if net == "pi" else Cph["q_part"][int(net[1:])][l])
        put("%s.dW%d.sum" % (net, l), K_RED, (part.sum(0), np.abs(part).sum(0), float(max(nch, 1))))
    return ops


def device(inp: dict) -> dict:
    """The device's (or simulate's) value of every output reference() names."""
    c, B = inp["case"], inp["B"]
    Aph, Cph = inp["actor"], inp["critic"]
    nt, L, NC, A, O = len(c.pi), len(c.q) + 1, c.NC, c.A, c.O
    d = {}
    for tag, ph in (("pi", Aph), ("pi'", Cph)):
        for l in range(nt): d["%s.h%d" % (tag, l)] = ph["t_act"][l]
        d[tag + ".mean"], d[tag + ".e"], d[tag + ".logp"] = ph["mean"], ph["e"], ph["logp"]
    d["pi.s"], d["pi.sd"], d["pi.a"] = Aph["s_s"], Aph["sd_s"], Aph["a_s"]
    d["pi'.a"] = Cph["xq_n"][:, O:O + A]
    for i in range(NC):
        for l in range(L):
            d["q%d.a.h%d" % (i, l)], d["q%d.c.h%d" % (i, l)], d["q%d.t.h%d" % (i, l)] = Aph["c_act"][i][l], Aph["c2_act"][i][l], Cph["c_act"][i][l]
            d["q%d.a.dy%d" % (i, l)], d["q%d.c.dy%d" % (i, l)] = Aph["c_dy"][i][l], Cph["c_dy"][i][l]
        if not c.fused: d["q%d.a.dxq" % i] = Aph["dxq"][i]
    d["pi.gmean"], d["pi.ge"] = Aph["gmean"], Aph["ge"]
    for l in range(nt): d["pi.dy%d" % l] = Aph["t_dy"][l]
    d["tgt"] = Cph["tgt"]
    if c.fused: d["lrow"] = Cph["lrow"]
    d["loss_actor"], d["loss_critic"] = Cph["scal"][1:2], Cph["scal"][0:1]
    Lp, Lq = layers(c, "pi"), layers(c, "q")
    for net, lay, parts, raw in [("pi", Lp, Cph["pi_part"], Cph["pi_grad"])] + [("q%d" % i, Lq, Cph["q_part"][i], Cph["q_grad"][i]) for i in range(NC)]:
        o = 0
        for l, (_, _, kp, np_, _) in enumerate(lay):
            for k_ in range(parts[l].shape[0]): d["%s.dW%d.part%d" % (net, l, k_)] = parts[l][k_]
            d["%s.dW%d.sum" % (net, l)] = raw[o:o + kp * np_ + np_]; o += kp * np_ + np_
    return d


def exact_checks(inp: dict):
    """What must hold bit for bit: the action in the critic input is the stored action, the packed columns are the batch's, everything
    outside the logical columns of the inputs is 0.  Returns a list of failure messages."""
    c = inp["case"]
    Aph, Cph, O, A = inp["actor"], inp["critic"], c.O, c.A
    bad = []
    eq = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    if not eq(Aph["xq_a"][:, O:O + A], Aph["a_s"][:, :A]): bad.append("xq_a's action columns are not the stored action")
    if not eq(Aph["xq_a"][:, :O], Aph["x_o"][:, :O]): bad.append("xq_a's observation columns are not x_o's")
    if not eq(Aph["xq_c"][:, :O], Aph["x_o"][:, :O]): bad.append("xq_c's observation columns are not x_o's")
    if not eq(Cph["xq_n"][:, :O], Cph["x_no"][:, :O]): bad.append("xq_n's observation columns are not x_no's")
    for k, m, w in (("x_o", Aph["x_o"], O), ("xq_a", Aph["xq_a"], O + A), ("xq_c", Aph["xq_c"], O + A), ("x_no", Cph["x_no"], O), ("xq_n", Cph["xq_n"], O + A)):
        if np.any(np.asarray(m)[:, w:] != 0): bad.append("%s: a padding column is not 0" % k)
    return bad


def branch_checks(inp: dict) -> list:
    """Non-vacuity on the buffers of `inp` (the device's, or simulate's): both ReLU states in every hidden layer, both `term` values,
    more than one selected critic where NC >= 2 (the tie case: every row ties and goes to critic 0, whose twin gets exactly 0), TD
    residuals on both sides of the SmoothL1 kink, and for the saturated case all three clamp states of s, an a == +-1.0f and one with
    0.995 < |a| < 1.  Returns the failures."""
    c = inp["case"]
    Aph, Cph, L, bad = inp["actor"], inp["critic"], len(c.q) + 1, []
    hidden = [("pi.h%d" % l, a, w) for l, (a, w) in enumerate(zip(Aph["t_act"], c.pi))] + [("pi'.h%d" % l, a, w) for l, (a, w) in enumerate(zip(Cph["t_act"], c.pi))]
    for i in range(c.NC):
        for tag, key, ph in (("a", "c_act", Aph), ("c", "c2_act", Aph), ("t", "c_act", Cph)):
            hidden += [("q%d.%s.h%d" % (i, tag, l), ph[key][i][l], c.q[l]) for l in range(L - 1)]
    for name, a, w in hidden:
        v = np.asarray(a)[:, :w]
        if not ((v > 0).any() and (v == 0).any()): bad.append("%s: one ReLU state only" % name)
    term = np.asarray(inp["term"])
    if not ((term == 0).any() and (term == 1).any()): bad.append("one `term` value only")
    qa = np.stack([np.asarray(Aph["c_act"][i][L - 1])[:, 0] for i in range(c.NC)])
    im, _ = select(qa)
    if c.special == "saturated":
        if not (c.NC >= 2 and (qa[0] == qa[1]).all() and (im == 0).all()): bad.append("not every row ties and goes to critic 0")
        if not (np.asarray(Aph["c_dy"][0][L - 1])[:, 0] == 1).all(): bad.append("critic 0 is not selected on every row")
        if any(np.asarray(x).any() for x in Aph["c_dy"][1]): bad.append("the unselected critic's gradient is not exactly 0")
        s, a = np.asarray(Aph["s_s"])[:, :c.A], np.asarray(Aph["a_s"], np.float32)[:, :c.A]
        if not ((s < f32(c.lo)).any() and ((s >= f32(c.lo)) & (s <= f32(c.hi))).any() and (s > f32(c.hi)).any()): bad.append("not all three clamp states of s")
        if not ((np.abs(a) == 1.0).any() and ((np.abs(a) > 0.995) & (np.abs(a) < 1)).any()): bad.append("no a == +-1.0f or none with 0.995 < |a| < 1")
    elif c.NC >= 2 and len(set(im.tolist())) < 2:
        bad.append("one critic is selected on every row")
    if c.loss == "SmoothL1":
        for i in range(c.NC):
            d = np.abs(np.asarray(Aph["c2_act"][i][L - 1], np.float32)[:, 0] - np.asarray(Cph["tgt"], np.float32))
            if not ((d < 1).any() and (d >= 1).any()): bad.append("q%d: TD residuals on one side of the SmoothL1 kink" % i)
    return bad


def kind(name: str) -> str:
    """an output's name without the critic and chunk numbers: q1.c.dy0 -> q.c.dy0, q2.dW1.part3 -> q.dW1.part.  The key of
    RESTATEMENT_RATIO / LAMBDA and of the GPU test's printed "sac layer ratios" line."""
    return re.sub(r"part\d+$", "part", re.sub(r"^q\d+", "q", name))


def lam_of(name: str) -> float:
    return LAMBDA[kind(name)]


def family(name: str) -> str:
    """the kernel form of an output: fwd (h*, mean, e), dx (dy*, dxq, gmean), dw (part*), red (sum), row (everything row-wise: lambda 1)."""
    t = name.split(".")[-1]
    if t.startswith("part"): return "dw"
    if t == "sum": return "red"
    if t.startswith("h") or t in ("mean", "e"): return "fwd"
    if t.startswith("dy") or t in ("dxq", "gmean"): return "dx"
    return "row"


# Criterion (c)'s factor per output (critics and chunks folded, see kind()): max(1, 4 x the largest |err| / (sqrt(n) u S) that the
# sequential float32 restatement reaches against f64 on the host inputs of every case.  `python tests/sac_layer_reference.py` prints
# the table; tests/test_sac_layer_reference.py recomputes all of it.  The 4 is for the device's accumulation order (four k-slices
# summed through LDS, row chunks, the four interleaved sums of the reduce) - it is NOT fitted to the device.  Row-wise outputs carry
# their whole bound in S: lambda 1, whatever their recorded ratio (which is that of simulate()'s f32 values, kept by the restatement).
RESTATEMENT_RATIO = {
    "loss_actor": 0.079, "loss_critic": 0.100, "lrow": 0.193, "pi'.a": 0.229, "pi'.e": 0.306,
    "pi'.h0": 1.129, "pi'.h1": 0.464, "pi'.h2": 0.183, "pi'.logp": 0.114, "pi'.mean": 0.434,
    "pi.a": 0.540, "pi.dW0.part": 1.051, "pi.dW0.sum": 0.707, "pi.dW1.part": 1.063, "pi.dW1.sum": 0.706,
    "pi.dW2.part": 0.860, "pi.dW2.sum": 0.705, "pi.dW3.part": 0.964, "pi.dW3.sum": 0.707, "pi.dW4.part": 0.909,
    "pi.dW4.sum": 0.000, "pi.dy0": 1.010, "pi.dy1": 0.685, "pi.dy2": 0.312, "pi.e": 0.303,
    "pi.ge": 0.454, "pi.gmean": 0.099, "pi.h0": 0.957, "pi.h1": 0.364, "pi.h2": 0.150,
    "pi.logp": 0.099, "pi.mean": 0.357, "pi.s": 0.332, "pi.sd": 0.319, "q.a.dxq": 0.662,
    "q.a.dy0": 0.514, "q.a.dy1": 0.424, "q.a.dy2": 0.426, "q.a.dy3": 0.000, "q.a.dy4": 0.000,
    "q.a.h0": 0.972, "q.a.h1": 0.446, "q.a.h2": 0.328, "q.a.h3": 0.256, "q.a.h4": 0.145,
    "q.c.dy0": 0.978, "q.c.dy1": 0.996, "q.c.dy2": 0.857, "q.c.dy3": 0.986, "q.c.dy4": 0.829,
    "q.c.h0": 1.051, "q.c.h1": 0.448, "q.c.h2": 0.368, "q.c.h3": 0.260, "q.c.h4": 0.115,
    "q.dW0.part": 0.946, "q.dW0.sum": 0.707, "q.dW1.part": 1.409, "q.dW1.sum": 0.707, "q.dW2.part": 1.469,
    "q.dW2.sum": 0.704, "q.dW3.part": 0.996, "q.dW3.sum": 0.000, "q.dW4.part": 0.613, "q.dW4.sum": 0.000,
    "q.t.h0": 0.883, "q.t.h1": 0.443, "q.t.h2": 0.317, "q.t.h3": 0.249, "q.t.h4": 0.154,
    "tgt": 0.371,
}
LAMBDA = {k: (1.0 if family(k) == "row" else max(1.0, 4.0 * v)) for k, v in RESTATEMENT_RATIO.items()}


# ------------------------------------------------------------------------------------------------ float32 restatement
def _acc(acc, prod64):
    return (acc.astype(np.float64) + prod64).astype(np.float32)


def _seq_mm(x, W, b=None):
    """x [M][K] @ W [K][N] (+ b) in f32, k sequential, products exact."""
    x64, W64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(W, np.float32).astype(np.float64)
    acc = np.zeros((x64.shape[0], W64.shape[1]), np.float32)
    for k in np.flatnonzero((x64 != 0).any(0) & (W64 != 0).any(1)):
        acc = _acc(acc, x64[:, k:k + 1] * W64[k][None, :])
    return acc if b is None else _acc(acc, np.asarray(b, np.float32).astype(np.float64)[None, :])


def _seq_dw(x, dy, r0, r1, skip=None):
    x64, dy64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(dy, np.float32).astype(np.float64)
    gw, gb = np.zeros((x64.shape[1], dy64.shape[1]), np.float32), np.zeros(dy64.shape[1], np.float32)
    for m in range(r0, r1):
        if m == skip: continue
        gw = _acc(gw, x64[m][:, None] * dy64[m][None, :]); gb = _acc(gb, dy64[m])
    return np.concatenate([gw.ravel(), gb])


def restatement(inp: dict, mut: Optional[str] = None) -> dict:
    """device(inp) with every GEMM output replaced by its sequential-f32 evaluation from the same inputs (row-wise outputs are kept:
    their formulas are restated by simulate()).  mut: one of MUTANTS - the wrong kernel of the host self-test."""
    c, B = inp["case"], inp["B"]
    Aph, Cph = inp["actor"], inp["critic"]
    Lp, Lq = layers(c, "pi"), layers(c, "q")
    nt, L, NC, A, O = len(c.pi), len(Lq), c.NC, c.A, c.O
    out = {k: np.array(v, np.float32) for k, v in device(inp).items()}
    relu = lambda v, on: np.maximum(v, np.float32(0)) if on else v
    def alias(x):   # the last row block's rows all read row B - 1 (a clamp `min(row, B - 1)` applied to the wrong index)
        if mut != "alias_last_block": return x
        x = np.array(x); x[(B - 1) // 32 * 32:] = x[B - 1]
        return x
    for tag, ph, P, x in (("pi", Aph, inp["pi0"], Aph["x_o"]), ("pi'", Cph, inp["pi1"], Cph["x_no"])):
        h = x
        for l in range(nt):
            out["%s.h%d" % (tag, l)] = relu(_seq_mm(alias(h) if tag == "pi" and l == 0 else h, *P[l]), True); h = ph["t_act"][l]
        out[tag + ".mean"], out[tag + ".e"] = _seq_mm(h, *P[nt]), _seq_mm(h, *P[nt + 1])
    for tag, ph, key, Ps, x in (("a", Aph, "c_act", inp["q"], Aph["xq_a"]), ("c", Aph, "c2_act", inp["q"], Aph["xq_c"]), ("t", Cph, "c_act", inp["qt"], Cph["xq_n"])):
        for i in range(NC):
            h = x
            for l in range(L):
                out["q%d.%s.h%d" % (i, tag, l)] = relu(_seq_mm(h, *Ps[i][l]), bool(Lq[l][4])); h = ph[key][i][l]
    mask = lambda v, m: np.where(np.asarray(m) > 0, v, np.float32(0))
    for i in range(NC):
        for l in range(L - 2, -1, -1):
            out["q%d.a.dy%d" % (i, l)] = mask(_seq_mm(Aph["c_dy"][i][l + 1], inp["q"][i][l + 1][0].T), Aph["c_act"][i][l])
            out["q%d.c.dy%d" % (i, l)] = mask(_seq_mm(Cph["c_dy"][i][l + 1], inp["q"][i][l + 1][0].T), Aph["c2_act"][i][l])
        if not c.fused: out["q%d.a.dxq" % i] = _seq_mm(Aph["c_dy"][i][0], inp["q"][i][0][0].T)
    P0 = inp["pi0"]
    v = _acc(_seq_mm(Aph["gmean"], P0[nt][0].T), _seq_mm(Aph["ge"], P0[nt + 1][0].T).astype(np.float64))
    out["pi.dy%d" % (nt - 1)] = mask(v, Aph["t_act"][nt - 1])
    for l in range(nt - 2, -1, -1):
        out["pi.dy%d" % l] = mask(_seq_mm(Aph["t_dy"][l + 1], P0[l + 1][0].T), Aph["t_act"][l])
    hin = Aph["t_act"][nt - 1]
    jobs = [("pi", l, x, dy, inp["pi_chunks"][l]) for l, (x, dy) in enumerate(zip([Aph["x_o"]] + list(Aph["t_act"][:nt - 1]) + [hin, hin], list(Aph["t_dy"]) + [Aph["gmean"], Aph["ge"]]))]
    for i in range(NC):
        jobs += [("q%d" % i, l, x, dy, inp["q_chunks"][l]) for l, (x, dy) in enumerate(zip([Cph["xq_c"]] + list(Aph["c2_act"][i][:L - 1]), Cph["c_dy"][i]))]
    for net, l, x, dy, nch in jobs:
        rows = dw_rows(c, B, nch)
        for k_, (r0, r1) in enumerate(rows):
            hit = mut == "drop_dw_row" and net == "q0" and l == 0 and k_ == len(rows) - 1
            out["%s.dW%d.part%d" % (net, l, k_)] = _seq_dw(x, dy, r0, r1, skip=(r1 - 1) if hit else None)
        part = np.asarray(Cph["pi_part"][l] if net == "pi" else Cph["q_part"][int(net[1:])][l], np.float32)
        acc = np.zeros(part.shape[1], np.float32)
        for k_ in range(part.shape[0]):
            if mut == "drop_reduce_chunk" and net == "q0" and l == 0 and k_ == part.shape[0] - 1 and part.shape[0] > 1: continue
            acc = _acc(acc, part[k_].astype(np.float64))
        out["%s.dW%d.sum" % (net, l)] = acc
    # ---- the other wrong kernels: applied to the values a correct kernel would have produced
    a, s, sd = (np.asarray(Aph[k], np.float64)[:, :A] for k in ("a_s", "s_s", "sd_s"))
    z = np.asarray(Aph["z"][0], np.float64)
    if mut == "shift_action_columns":      # d qmin / d a read one column to the right
        alpha = np.exp(np.float64(Aph["log_alpha"][0]))
        dq = sum(_d(Aph["c_dy"][i][0]) @ _d(inp["q"][i][0][0]).T for i in range(NC))[:, O + 1:O + A + 1]
        out["pi.gmean"][:, :A] = (((alpha * 2 * a / ((1 - a * a) + f32(c.eps))) - dq) / B * (1 - a * a)).astype(np.float32)
    if mut == "tie_to_higher":
        qa = np.stack([np.asarray(Aph["c_act"][i][L - 1])[:, 0] for i in range(NC)])
        im = (NC - 1) - np.argmin(qa[::-1], 0)
        for i in range(NC):
            out["q%d.a.dy%d" % (i, L - 1)][:, 0] = (im == i)
    if mut == "ignore_inr":
        out["pi.ge"][:, :A] = (np.asarray(Aph["gmean"], np.float64)[:, :A] * z * sd * s).astype(np.float32)
    if mut == "drop_eps":
        out["pi.logp"] = ((-LN_SQRT_2PI - 0.5 * z * z).sum(1) - np.log(np.maximum(1 - a * a, 1e-300)).sum(1)).astype(np.float32)
    if mut == "target_from_old_actor":     # a' and log p' of the actor BEFORE its step
        old = simulate(c, inp["_flat"]["pi"], inp["_flat"]["q"], inp["_flat"]["qt"], inp["_flat"]["batch"], inp["_flat"]["log_alpha"], np.float32)
        out["pi'.mean"], out["pi'.e"], out["pi'.logp"] = old["critic"]["mean"], old["critic"]["e"], old["critic"]["logp"]
        out["pi'.a"] = old["critic"]["xq_n"][:, O:O + A]
    if mut == "padding_nonzero":
        out["pi.mean"][0, A] = np.float32(1e-30)
    return out


MUTANTS = ("drop_dw_row", "drop_reduce_chunk", "alias_last_block", "shift_action_columns", "tie_to_higher", "ignore_inr", "drop_eps",
           "target_from_old_actor", "padding_nonzero")


def verdicts(ops: dict, dev: dict) -> dict:
    return {k: check(ops[k], dev[k], lam_of(k)) for k in ops}


def failures(ops: dict, dev: dict) -> list:
    return [v.message for v in verdicts(ops, dev).values() if not v.ok]


def kind_ratios(ops: dict, dev: dict, by=kind) -> dict:
    """largest |err| / (sqrt(n) u S) per output (critics and chunks folded: the figure lambda is set from, and the GPU test's printed
    line), or per kernel family (by=family)."""
    out = {}
    for k in ops:
        r = check(ops[k], dev[k], np.inf).sharp_ratio
        out[by(k)] = max(out.get(by(k), 0.0), r)
    return out


def function_errors(inp: dict) -> dict:
    """largest error of the device's expf / tanhf / logf in units of u relative to the result, against f64 libm on the same f32
    argument, from the stored stages of the actor phase.  tanhf: the argument is sd z + mean as one fma or as a rounded product and
    an add - the candidate closer to the device's value counts.  logf: only where act_dim == 1 (log p is then one log term; the
    figure includes the final subtraction's rounding, an over-estimate)."""
    c = inp["case"]; A = c.A
    Aph = inp["actor"]
    e, s, sd, a, mean = (np.asarray(Aph[k], np.float32)[:, :A] for k in ("e", "s_s", "sd_s", "a_s", "mean"))
    z = np.asarray(Aph["z"][0], np.float32)
    out = {}
    r = np.exp(_d(e)); out["expf"] = float((np.abs(_d(s) - r) / (U * r)).max())
    cl = np.clip(s, np.float32(f32(c.lo)), np.float32(f32(c.hi))); r = np.exp(_d(cl)); out["expf"] = max(out["expf"], float((np.abs(_d(sd) - r) / (U * r)).max()))
    t_fma = (_d(sd) * _d(z) + _d(mean)).astype(np.float32)
    t_two = ((sd * z).astype(np.float32) + mean).astype(np.float32)
    err = np.minimum(*[np.abs(_d(a) - np.tanh(_d(t))) / (U * np.maximum(np.abs(np.tanh(_d(t))), 1e-300)) for t in (t_fma, t_two)])
    out["tanhf"] = float(err.max())
    if A == 1:
        # log p = fl(nl - sl), sl = logf(w).  On rows with |nl - lp| >= |lp| the f32 sl is known exactly: sl = nl - lp (the subtraction
        # of the kernel was exact there, its result being no larger than an operand of the same sign pattern), so logf's own
        # error is observable.  nl and w each have two forms (contracted or not); the pair closest to the device counts.
        lp = _d(Aph["logp"])
        best, valid = None, None
        for aa in ((a * a).astype(np.float32), None):
            om = (np.float32(1) - aa).astype(np.float32) if aa is not None else (1 - _d(a) * _d(a)).astype(np.float32)
            w = (om + np.float32(f32(c.eps))).astype(np.float32)[:, 0]
            for nl in ((np.float32(-LN_SQRT_2PI) - (np.float32(0.5) * (z * z).astype(np.float32)).astype(np.float32)).astype(np.float32)[:, 0],
                       (-LN_SQRT_2PI - 0.5 * _d((z * z).astype(np.float32))).astype(np.float32)[:, 0]):
                sl = _d(nl) - lp
                ok = (np.abs(sl) >= np.abs(lp)) & (sl.astype(np.float32).astype(np.float64) == sl)
                er = np.where(ok, np.abs(sl - np.log(_d(w))) / (U * np.maximum(np.abs(np.log(_d(w))), 1e-300)), np.inf)
                best = er if best is None else np.minimum(best, er)
        valid = np.isfinite(best)
        if valid.sum() >= 8:
            out["logf"] = float(best[valid].max())
            out["logf_rows"] = float(valid.sum())
    return out


def host_inputs(c: Case, B: Optional[int] = None, dtype=np.float32, chunks: Optional[int] = None, step: int = 0):
    """simulate() on the case's own parameters and batch, with the flat inputs kept for the mutants.  The actor 'after its step' is the
    actor moved by 1e-3 x a fixed direction (the host does not model Adam; the critic phase only needs that it differs)."""
    B = B or c.B
    pi, qs = case_params(c)
    batch = case_batch(c, B, step)
    la = 0.0 if c.ent[0] == "Auto" else math.log(c.ent[1])
    pi1 = (pi + np.float32(1e-3) * np.sign(np.sin(np.arange(pi.size, dtype=np.float32)))).astype(np.float32)
    if chunks is None:
        chunks = max(1, min(16, B // 256)) if c.small else max(1, min(16, B // 64))   # (64x64 tiles: one tile per layer in the case that takes them, so the plan's tile cap does not bind)
    inp = simulate(c, pi, qs, qs, batch, la, dtype, chunks=chunks, pi1_flat=pi1)
    inp["_flat"] = dict(pi=pi, q=qs, qt=qs, batch=batch, log_alpha=la, pi1=pi1)
    return inp


def table_text(ratio: dict, per_line: int = 5) -> str:
    items = ['"%s": %.3f' % kv for kv in sorted(ratio.items())]
    return "\n".join("    " + ", ".join(items[i:i + per_line]) + "," for i in range(0, len(items), per_line))


if __name__ == "__main__":   # the restatement's ratios on the host inputs of every case: sets RESTATEMENT_RATIO
    worst = {}
    for c in CASES.values():
        inp = host_inputs(c)
        r = kind_ratios(reference(inp), restatement(inp))
        print(c.name, " ".join("%s %.3f" % kv for kv in sorted(r.items())), flush=True)
        for k, v in r.items(): worst[k] = max(worst.get(k, 0.0), v)
    print("RESTATEMENT_RATIO = {\n" + table_text(worst) + "\n}")
