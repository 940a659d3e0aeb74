"""Float64 reference, float32 restatement and cases of the Mlp DQN step's kernels, one layer at a time (csrc/mlp_agents.hip
DqnMlp::update_critic, csrc/mlp_fused.hpp, csrc/dense.hpp).  Written beside tests/sac_layer_reference.py, whose generic helpers (_op,
_fwd, _dx, _dw, _seq_mm, kind_ratios, table_text) it imports; Op and check are those of tests/dqn_backward_reference.py.  Nothing
under border_amd/ imports this file.

Given the device's own inputs of a kernel (Dqn.layer: every raw buffer of the last update, padding included; the parameter arenas as
they stood before the step) each output is one of

  a GEMM output    reference(inp): name -> Op with the f64 value of that layer alone, S = sum |a_k| |b_k| and the reduction length n.
                   ReLU masks come from the probed activations (`> 0`), so no element is exempt.  Criteria: (a) S == 0 -> exactly 0
                   (every padding row and column, masked units, an empty row chunk, the gradient arena's padding);  (b) |err| <= n u S;
                   (c) |err| <= lambda sqrt(n) u S, u = 2^-24, lambda = LAMBDA[kind(name)] = max(1, 4 x RESTATEMENT_RATIO): the largest
                   ratio of the sequential-f32 restatement on the host inputs of every case, computed on the CPU, never fitted to a device.
  a row output     exact(inp): name -> the f32 bits.  The pack (the input rows' bits, zeros beyond in_dim), and the row arithmetic as a
                   fixed sequence of IEEE f32 operations from the probed Q rows: first-max argmax (lowest index on a tie), td_target and
                   td_loss_row of csrc/agent_base.hpp (contraction is off there) for both loss kinds and the weighted / clipped branch,
                   dq = dl / B (zeroed where activation_out clamps the selected Q), the one-hot dy[L-1] row, and the loss mean in
                   k_mean_rows' order: strided per-thread sums, then the 256-wide tree.  The 512-thread tree of the one-workgroup step
                   and the shuffle tree of the LDS step add only zeros beyond it.  ONE operation differs between the forms and is
                   restated per form: the one-workgroup kernels finish the mean with a division, red[0] / (float)B, the layer path
                   (k_mean_rows, k_mlp_head_td) with a product, red[0] * (1.0f / (float)B).  Both are single IEEE operations, so
                   each form is still held bit for bit - but the recorded loss of a shape differs by up to 1 ulp between the forms
                   wherever B is no power of two.
  the optimizer    the parameters and moments after the step are optimizer_inputs.adam_f32 of the read-back gradient arena, bit for bit
                   (parameters: one of the three roots of optimizer_inputs.SQRT_ULPS, the bar of tests/test_gpu_optimizer_edges.py);
                   the target arena does not move (the cases never reach a soft update); every padding element stays exactly 0.

Ops and the `__global__` entries they name (the step form decides):
  pack             k_dqn_mlp_step_lds | k_dqn_mlp_step | k_mlp_pack_z | pack_rows
  z{z}.h{l}        the same two one-workgroup entries | k_dense_small<false> | k_mlp_head_td (last layer under the head) | k_igemm
  rows, dy{L-1}    one-workgroup entries | k_mlp_head_td | k_td_dense;  loss: ... | k_mlp_head_td | k_mean_rows
  dy{l}, l < L-1   one-workgroup entries | k_dense_small<true> | k_mlp_head_td (dy{L-2} under the head) | k_igemm
  gW{l}.part{k}    k_dense_dw_small_group, rows [k per, min(B, (k + 1) per)), per = ceil(ceil(B / chunks) / 32) * 32; gb is its tail
  gW{l}.sum        k_dense_reduce_adam: the launched chunks' partials into the gradient arena
  gW{l}            straight into the arena: one-workgroup entries | k_igemm_red<DenseDw> + k_dense_reduce (64x64 tiles)
  adam             one-workgroup entries | k_dense_reduce_adam | launch_adam

Tie cases.  Under double DQN the selector is the online network on next_obs: its two columns are bit-identical (every row ties), the
target's two columns are NOT, so the index the tie resolves to decides the target value.  Without double DQN the selector is the
target network itself and both of its columns are identical: every row ties, and either index reads the same value - the case holds the
kernels to its bits, the mutant is only observable under double DQN.

Layouts are the device's: W [Kp][Np] k-major then bias [Np] per layer in an arena, activations [B][Np], all sizes padded to 64."""
from __future__ import annotations

import math
import os
import re
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimizer_inputs as OI  # noqa: E402
from dqn_backward_reference import U, check  # noqa: E402,F401
from group_layers_restatement import Shape, fused_ok  # noqa: E402
from sac_layer_reference import _acc, _d, _dw, _dx, _fwd, _op, _seq_mm, f32, kind_ratios, pad64, table_text  # noqa: E402,F401

F32 = np.float32
FORMS = ("lds", "global", "layers_head", "layers_td", "tiles")
LR = 1e-3
GAMMA = 0.99


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    in_dim: int
    units: tuple
    A: int
    batches: tuple                  # batch sizes of the updates on one agent
    double: bool = False
    loss: str = "Mse"
    env: tuple = ()
    act_out: bool = False           # MlpConfig::activation_out
    weighted: bool = False          # importance weights and clip_td_err
    clip: tuple = (0.5, 2.0)
    special: str = ""               # "tie" | "all-terminal"
    seed: int = 0
    one_wg: bool = False            # the case is there for the one-workgroup step (run by default and with BDR_NO_MLP_LDS=1)

    @property
    def L(self) -> int:
        return len(self.units) + 1

    @property
    def nz(self) -> int:
        return 3 if self.double else 2

    @property
    def capacity(self) -> int:      # the agent's batch_size: what ensure_batch allocates at creation
        return max(self.batches)


CASES = {c.name: c for c in (
    # ---- one workgroup
    Case("c1-double", 4, (64, 64), 2, (32,), double=True, loss="SmoothL1", special="tie", seed=1, one_wg=True),
    Case("two-blocks", 4, (64, 64), 2, (64,), special="all-terminal", seed=2, one_wg=True),
    Case("ragged-lds", 4, (64, 64), 2, (48,), loss="SmoothL1", weighted=True, seed=3, one_wg=True),
    Case("ragged-deep", 7, (64, 64, 64), 5, (33,), seed=4, one_wg=True),
    Case("one-row", 3, (64,), 3, (1,), loss="SmoothL1", seed=5, one_wg=True),
    Case("wide-in", 100, (64,), 33, (17,), seed=6, one_wg=True),
    Case("wide-hidden", 5, (128,), 6, (32,), act_out=True, seed=7, one_wg=True),
    Case("a64-double", 4, (64,), 64, (32,), double=True, seed=8, one_wg=True),
    # ---- layer by layer
    Case("l-65", 4, (64, 64), 2, (65,), special="tie", seed=9),
    Case("l-65-double", 4, (64, 64), 2, (65,), double=True, loss="SmoothL1", special="tie", seed=10),
    Case("l-wide-head", 6, (64, 192), 5, (33,), act_out=True, seed=11),
    Case("l-wide-head-fused", 6, (64, 192), 5, (33,), act_out=True, env=(("BDR_MLP_HEAD_FUSE_WIDE", "1"),), seed=11),
    Case("l-a33", 9, (96,), 33, (40,), weighted=True, seed=12),
    Case("l-a64-double", 4, (64,), 64, (33,), double=True, loss="SmoothL1", seed=13),
    # (40 rows of this net fit the one-workgroup step: the last update of l-chunks leaves the layer path, and the gradient arena is then
    #  written without partials.  l-chunks-layers keeps the agent on the layer path - 40 rows: planned 16 chunks, launched 1)
    Case("l-chunks", 11, (64, 64), 3, (515, 4100, 40), loss="SmoothL1", seed=14),
    Case("l-chunks-layers", 11, (64, 64), 3, (515, 4100, 40), loss="SmoothL1", env=(("BDR_NO_MLP_FUSED", "1"),), seed=14),
    Case("l-deep", 3, (64, 128, 64, 96, 64, 64, 32, 64), 4, (33,), seed=15),
    Case("l-wide-k", 5, (512, 64), 2, (33,), seed=16),
    Case("l-big-tiles", 4, (128, 96), 3, (130,), env=(("BDR_NO_SMALL_GEMM", "1"),), seed=17),
)}


def layers(c: Case):
    """(in, out, Kp, Np, relu) per layer"""
    w = (c.in_dim,) + tuple(c.units) + (c.A,)
    return [(i, o, pad64(i), pad64(o), 1 if l < c.L - 1 else int(c.act_out)) for l, (i, o) in enumerate(zip(w[:-1], w[1:]))]


def total(c: Case) -> int:
    return sum(kp * np_ + np_ for (_, _, kp, np_, _) in layers(c))


def shapes(c: Case):
    return [s for (i, o, _, _, _) in layers(c) for s in ((o, i), (o,))]


def to_arena(flat, c: Case):
    """reference order (weight [out][in], bias [out] per layer) -> the padded arena, dtype kept"""
    flat = np.asarray(flat)
    out, o = [], 0
    for (i, n, kp, np_, _) in layers(c):
        W = np.zeros((kp, np_), flat.dtype); b = np.zeros(np_, flat.dtype)
        W[:i, :n] = flat[o:o + n * i].reshape(n, i).T; o += n * i
        b[:n] = flat[o:o + n]; o += n
        out += [W.ravel(), b]
    return np.concatenate(out)


def arena(c: Case, raw):
    """a raw padded arena -> [(W [Kp][Np], b [Np])] (views)"""
    out, o = [], 0
    for (_, _, kp, np_, _) in layers(c):
        out.append((raw[o:o + kp * np_].reshape(kp, np_), raw[o + kp * np_:o + kp * np_ + np_])); o += kp * np_ + np_
    return out


def real_mask(c: Case):
    """True where an arena element belongs to the logical network"""
    out = []
    for (i, n, kp, np_, _) in layers(c):
        W = np.zeros((kp, np_), bool); b = np.zeros(np_, bool)
        W[:i, :n] = True; b[:n] = True
        out += [W.ravel(), b]
    return np.concatenate(out)


def case_params(c: Case):
    """qnet, qnet_tgt flat f32 in reference order, seeded and scaled as sac_layer_reference.case_params; the two differ."""
    def init(seed):
        rng, out, fan = np.random.default_rng(seed), [], 1
        for s in shapes(c):
            if len(s) > 1: fan = s[1]
            out.append((rng.uniform(-1, 1, s) / math.sqrt(fan)).astype(F32).ravel())
        return out
    q, qt = init(1000 + c.seed), init(2000 + 10 * c.seed)
    if c.special == "tie":   # output columns 0 and 1 bit-identical: the online network always, the target unless it is not the selector
        for p in ([q] if c.double else [q, qt]):
            W = p[-2].reshape(c.A, -1); W[1] = W[0]; p[-1][1] = p[-1][0]
    return np.concatenate(q), np.concatenate(qt)


def case_batch(c: Case, B: int, step: int = 0):
    """obs, act, next_obs, reward, is_terminated, weight (None unless the case is weighted).  Action 0 has no row; every other row takes
    action A - 1 (at least 17 rows of it from B = 33 on)."""
    rng = np.random.default_rng(3000 + 100 * c.seed + step)
    obs = rng.standard_normal((B, c.in_dim)).astype(F32)
    nobs = rng.standard_normal((B, c.in_dim)).astype(F32)
    act = (rng.integers(1, c.A, B) if c.A > 1 else np.zeros(B)).astype(np.int64)
    act[::2] = c.A - 1
    rew = (rng.standard_normal(B) * 2).astype(F32)
    term = np.ones(B, np.int8) if c.special == "all-terminal" else (np.arange(B) % 4 == 1).astype(np.int8)
    w = rng.uniform(0.2, 1.5, B).astype(F32) if c.weighted else None
    return obs, act, nobs, rew, term, w


def lds_bytes(c: Case, B: int) -> int:
    """mf_lds_plan (csrc/mlp_fused.hpp): rows padded by 4 floats; 0 when the plan exceeds 150 KB"""
    lay = layers(c)
    maxw = max([lay[0][2]] + [l[3] for l in lay])
    o = B * (lay[0][2] + 4) + 2 * sum(B * (l[3] + 4) for l in lay) + (c.nz - 1) * 2 * B * (maxw + 4)
    return 4 * o if 4 * o <= 150 * 1024 else 0


def predict_form(c: Case, B: int, env=()) -> str:
    env = dict(tuple(c.env) + tuple(env))
    s = Shape(c.in_dim, c.units, c.A, B, double_dqn=c.double)
    if "BDR_NO_MLP_FUSED" not in env and fused_ok(s):
        return "lds" if "BDR_NO_MLP_LDS" not in env and lds_bytes(c, B) else "global"
    if env.get("BDR_NO_SMALL_GEMM") == "1":
        return "tiles"
    head = "BDR_NO_MLP_HEAD_FUSE" not in env and c.L >= 2 and c.A <= 32 and s.Kp[-1] <= (4096 if "BDR_MLP_HEAD_FUSE_WIDE" in env else 128)
    return "layers_head" if head else "layers_td"


def predict_chunks(c: Case, B: int, form: str) -> int:
    """the row chunks of the grouped weight gradient (0: the form makes no partials): planned for the capacity, launched for B"""
    if not form.startswith("layers"): return 0
    return min(max(1, min(16, c.capacity // 256)), max(1, B // 256))


def dw_rows(B: int, chunks: int):
    """k_dense_dw_small_group's row ranges (an empty one has r0 >= r1)"""
    per = ((B + chunks - 1) // chunks + 31) // 32 * 32
    return [(k * per, max(k * per, min(B, (k + 1) * per))) for k in range(chunks)]


# ------------------------------------------------------------------------------------------------ row arithmetic, bit for bit
def first_argmax(q, A):
    """lowest index of the maximum over the A real columns"""
    return np.argmax(np.asarray(q)[:, :A], axis=1)


def mean_rows(x, B, form, dt=F32):
    """k_mean_rows: 256 strided per-thread sums, the 256-wide tree, then the form's last operation"""
    red = np.zeros(256, dt)
    for b in range(B):
        red[b % 256] = dt(red[b % 256] + x[b])
    w = 128
    while w > 0:
        red[:w] = (red[:w] + red[w:2 * w]).astype(dt); w >>= 1
    if form in ("lds", "global"):
        return dt(red[0] / dt(B))
    return dt(red[0] * dt(dt(1.0) / dt(B)))


def rows_step(c: Case, B: int, form: str, q_on, q_tg, q_nx, act, rew, term, weight, dt=F32, mut: Optional[str] = None):
    """k_td_dense / the TD phase of the one-workgroup kernels / of k_mlp_head_td as a fixed sequence of operations in `dt` (float32: the
    device's bits; float64: the exact chain of the host's autograd comparison).  q_*: the probed Q rows [B][Np]."""
    A, ld = c.A, q_on.shape[1]
    q_on, q_tg = np.asarray(q_on, dt), np.asarray(q_tg, dt)
    sel = np.asarray(q_nx, dt) if c.double else q_tg
    if mut == "selector_from_target": sel = q_tg
    idx = first_argmax(sel, A)
    if mut == "tie_to_higher": idx = (A - 1) - np.argmax(sel[:, :A][:, ::-1], axis=1)
    r = np.arange(B)
    qn, pred = q_tg[r, idx], q_on[r, act]
    with np.errstate(all="ignore"):
        k = ((1 - np.asarray(term, np.int64)).astype(dt) * dt(f32(GAMMA))).astype(dt)
        tgt = (np.asarray(rew, dt) + (k * qn).astype(dt)).astype(dt)
        d = (pred - tgt).astype(dt)
        smooth = c.loss == "SmoothL1"
        if weight is None:
            td = np.abs(d)
            if smooth:
                z = np.abs(d)
                lossb = np.where(z < 1, ((dt(0.5) * z).astype(dt) * z).astype(dt), (z - dt(0.5)).astype(dt))
                dl = np.where(z < 1, d, np.where(d > 0, dt(1), dt(-1)))
            else:
                lossb, dl = (d * d).astype(dt), (dt(2) * d).astype(dt)
        else:
            w = np.asarray(weight, dt)
            raw = np.abs(d)
            cmin, cmax = dt(f32(c.clip[0])), dt(f32(c.clip[1]))
            td = np.minimum(np.maximum(raw, cmin), cmax)
            pas = ((raw >= cmin) & (raw <= cmax)).astype(dt)
            x = (w * td).astype(dt)
            if smooth:
                z = np.abs(x)
                lossb = np.where(z < 1, ((dt(0.5) * z).astype(dt) * z).astype(dt), (z - dt(0.5)).astype(dt))
                dx = np.where(z < 1, x, np.where(x > 0, dt(1), dt(-1)))
            else:
                lossb, dx = (x * x).astype(dt), (dt(2) * x).astype(dt)
            sgn = np.where(d > 0, dt(1), np.where(d < 0, dt(-1), dt(0)))
            dl = (((dx * w).astype(dt) * pas).astype(dt) * sgn).astype(dt)
        dq = (dl.astype(dt) / dt(B)).astype(dt)
        if c.act_out and mut != "keep_clamped_gradient":
            dq = np.where(pred > 0, dq, dt(0))
    dy = np.zeros((B, ld), dt); dy[r, act] = dq
    return dict(pred=pred, tgt=tgt, loss_row=lossb.astype(dt), td_abs=td.astype(dt), dy_last=dy,
                loss=np.array([mean_rows(lossb.astype(dt), B, form, dt)], dt), idx=idx)


# ------------------------------------------------------------------------------------------------ the step on the host
def simulate(c: Case, B: int, q_flat, qt_flat, batch, form: str, chunks: int, dtype=F32, t: int = 1):
    """Every buffer Dqn.layer returns, computed on the host in `dtype` (float32: what the device would hold up to summation order;
    float64: the exact chain).  Returns the `inp` of reference() / exact()."""
    obs, act, nobs, rew, term, weight = batch
    lay = layers(c); L, nz = c.L, c.nz
    f = lambda x: np.asarray(x, dtype)
    mm = lambda a_, b_: (np.asarray(a_, np.float64) @ np.asarray(b_, np.float64)).astype(dtype)
    q0, qt0 = to_arena(f(q_flat), c), to_arena(f(qt_flat), c)
    P, PT = arena(c, q0), arena(c, qt0)

    def packed(x):
        o = np.zeros((B, lay[0][2]), dtype); o[:, :c.in_dim] = x; return o
    x_in = [packed(f(obs)), packed(f(nobs)), packed(f(nobs))][:nz]
    acts = []
    for z in range(nz):
        h, a_ = x_in[z], []
        for l in range(L):
            Wb = (PT if z == 1 else P)[l]
            h = mm(h, Wb[0]) + Wb[1]
            if lay[l][4]: h = np.maximum(h, 0)
            a_.append(h.astype(dtype))
        acts.append(a_)
    rows = rows_step(c, B, form, acts[0][L - 1], acts[1][L - 1], acts[2][L - 1] if c.double else None, act, rew, term, weight, dtype)
    dy = [None] * L
    dy[L - 1] = rows["dy_last"]
    for l in range(L - 2, -1, -1):
        dy[l] = (mm(dy[l + 1], P[l + 1][0].T) * (acts[0][l] > 0)).astype(dtype)
    xs = [x_in[0]] + acts[0][:L - 1]
    part, grad = [], []
    for l in range(L):
        rr = dw_rows(B, chunks) if chunks else [(0, B)]
        p = np.stack([np.concatenate([mm(xs[l][r0:r1].T, dy[l][r0:r1]).ravel(), dy[l][r0:r1].astype(np.float64).sum(0).astype(dtype)]) for r0, r1 in rr])
        part.append(p); grad.append(p.astype(np.float64).sum(0).astype(dtype))
    inp = dict(case=c, B=B, form=form, chunks=chunks, t=t, obs=f(obs), nobs=f(nobs), act=np.asarray(act), reward=f(rew), term=np.asarray(term),
               weight=None if weight is None else f(weight), q0=q0, qt0=qt0, m0=np.zeros_like(q0), v0=np.zeros_like(q0),
               x_in=x_in, acts=acts, dy=dy, pred=rows["pred"], tgt=rows["tgt"], loss_row=rows["loss_row"], td_abs=rows["td_abs"], loss=rows["loss"],
               part=part if chunks else None, grad=np.concatenate(grad))
    if dtype == F32:
        s = OI.adam_scalars(False, LR, 0.9, 0.999, 1e-8, 0.0, t)
        inp["q1"], inp["m1"], inp["v1"], _ = OI.adam_f32(q0, inp["grad"], inp["m0"], inp["v0"], None, s)
        inp["qt1"] = qt0.copy()
    return inp


def host_inputs(c: Case, step: int = 0, dtype=F32, env=()):
    B = c.batches[step]
    form = predict_form(c, B, env)
    q, qt = case_params(c)
    return simulate(c, B, q, qt, case_batch(c, B, step), form, predict_chunks(c, B, form), dtype, t=step + 1)


# ------------------------------------------------------------------------------------------------ reference and device values
def kernels(form: str) -> dict:
    one = {"lds": "k_dqn_mlp_step_lds", "global": "k_dqn_mlp_step"}.get(form)
    if one:
        return dict(pack=one, fwd=one, head=one, rows=one, loss=one, dx=one, dx_head=one, dw=one, adam=one)
    if form == "tiles":
        return dict(pack="pack_rows", fwd="k_igemm", head="k_igemm", rows="k_td_dense", loss="k_mean_rows", dx="k_igemm", dx_head="k_igemm",
                    dw="k_igemm_red<DenseDw> | k_dense_reduce", adam="launch_adam")
    h = form == "layers_head"
    return dict(pack="k_mlp_pack_z", fwd="k_dense_small<false>", head="k_mlp_head_td" if h else "k_dense_small<false>",
                rows="k_mlp_head_td" if h else "k_td_dense", loss="k_mlp_head_td" if h else "k_mean_rows", dx="k_dense_small<true>",
                dx_head="k_mlp_head_td" if h else "k_dense_small<true>", part="k_dense_dw_small_group", red="k_dense_reduce_adam",
                adam="k_dense_reduce_adam")


def reference(inp: dict) -> dict:
    """name -> Op for every GEMM output of one update"""
    c, B = inp["case"], inp["B"]
    lay = layers(c); L, K = c.L, kernels(inp["form"])
    P, PT = arena(c, inp["q0"]), arena(c, inp["qt0"])
    ops = {}
    for z in range(c.nz):
        h = inp["x_in"][z]
        for l in range(L):
            name = "z%d.h%d" % (z, l)
            ops[name] = _op(name, K["head"] if l == L - 1 else K["fwd"], *_fwd(h, (PT if z == 1 else P)[l], lay[l][0], bool(lay[l][4])))
            h = inp["acts"][z][l]
    for l in range(L - 2, -1, -1):
        name = "dy%d" % l
        ops[name] = _op(name, K["dx_head"] if l == L - 2 else K["dx"], *_dx(inp["dy"][l + 1], P[l + 1][0], inp["acts"][0][l]))
    xs = [inp["x_in"][0]] + list(inp["acts"][0][:L - 1])
    for l in range(L):
        if inp["chunks"]:
            for k, (r0, r1) in enumerate(dw_rows(B, inp["chunks"])):
                name = "gW%d.part%d" % (l, k)
                ops[name] = _op(name, K["part"], *_dw(xs[l], inp["dy"][l], r0, r1))
            part = _d(inp["part"][l])
            ops["gW%d.sum" % l] = _op("gW%d.sum" % l, K["red"], part.sum(0), np.abs(part).sum(0), float(inp["chunks"]))
        else:
            ops["gW%d" % l] = _op("gW%d" % l, K["dw"], *_dw(xs[l], inp["dy"][l], 0, B))
    return ops


def grad_segments(c: Case, raw):
    out, o = [], 0
    for (_, _, kp, np_, _) in layers(c):
        out.append(raw[o:o + kp * np_ + np_]); o += kp * np_ + np_
    return out


def device(inp: dict) -> dict:
    """The device's (or simulate's) value of every output reference() and exact() name."""
    c, L = inp["case"], inp["case"].L
    d = {"pack.z%d" % z: inp["x_in"][z] for z in range(c.nz)}
    for z in range(c.nz):
        for l in range(L): d["z%d.h%d" % (z, l)] = inp["acts"][z][l]
    for l in range(L - 1): d["dy%d" % l] = inp["dy"][l]
    d["dy%d" % (L - 1)] = inp["dy"][L - 1]
    for k in ("pred", "tgt", "loss_row", "td_abs", "loss"): d[k] = inp[k]
    seg = grad_segments(c, inp["grad"])
    for l in range(L):
        if inp["chunks"]:
            for k in range(inp["chunks"]): d["gW%d.part%d" % (l, k)] = inp["part"][l][k]
            d["gW%d.sum" % l] = seg[l]
        else:
            d["gW%d" % l] = seg[l]
    for k in ("q1", "m1", "v1", "qt1"): d["adam." + k] = inp[k]
    return d


def exact(inp: dict, mut: Optional[str] = None) -> dict:
    """name -> [candidate f32 arrays]: the device's value must carry the bits of one candidate, element by element."""
    c, B, L = inp["case"], inp["B"], inp["case"].L
    out = {}
    for z in range(c.nz):
        x = np.zeros((B, layers(c)[0][2]), F32); x[:, :c.in_dim] = inp["nobs" if z else "obs"]
        out["pack.z%d" % z] = [x]
    r = rows_step(c, B, inp["form"], inp["acts"][0][L - 1], inp["acts"][1][L - 1], inp["acts"][2][L - 1] if c.double else None, inp["act"], inp["reward"],
                  inp["term"], inp["weight"], F32, mut)
    for k in ("pred", "tgt", "loss_row", "td_abs", "loss"): out[k] = [r[k]]
    out["dy%d" % (L - 1)] = [r["dy_last"]]
    s = OI.adam_scalars(False, LR, 0.9, 0.999, 1e-8, 0.0, inp["t"])
    cand = [OI.adam_f32(inp["q0"], inp["grad"], inp["m0"], inp["v0"], None, s, u) for u in OI.SQRT_ULPS]
    q1, m1, v1 = [x[0] for x in cand], cand[0][1], cand[0][2]
    if mut == "adam_skips_vector":   # the last real row of W_0, its first four columns: parameters and moments left as they were
        o = (c.in_dim - 1) * layers(c)[0][3]
        q1 = [x.copy() for x in q1]; m1, v1 = m1.copy(), v1.copy()
        for x, x0 in [(x, inp["q0"]) for x in q1] + [(m1, inp["m0"]), (v1, inp["v0"])]: x[o:o + 4] = x0[o:o + 4]
    out["adam.q1"], out["adam.m1"], out["adam.v1"], out["adam.qt1"] = q1, [m1], [v1], [inp["qt0"]]
    return out


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


def exact_failures(ex: dict, dev: dict) -> list:
    bad = []
    for k, cands in ex.items():
        got = bits(dev[k]).reshape(bits(cands[0]).shape)
        ok = np.zeros(got.shape, bool)
        for w in cands: ok |= got == bits(w)
        # (+0 and -0: a sum of exact zeros may carry either sign only where the restatement says so; none of these outputs does)
        if not ok.all():
            i = np.unravel_index(int(np.argmin(ok)), ok.shape)
            bad.append("%s: %d of %d elements differ in bits from the f32 restatement; first at %s: device %r, expected %r"
                       % (k, (~ok).sum(), ok.size, i, np.asarray(dev[k], F32).reshape(ok.shape)[i], np.asarray(cands[0], F32)[i]))
    return bad


def padding_failures(inp: dict) -> list:
    pad = ~real_mask(inp["case"])
    return ["%s: %d padding elements are not exactly 0" % (k, np.count_nonzero(np.asarray(inp[k])[pad]))
            for k in ("q1", "qt1", "m1", "v1", "grad") if np.any(np.asarray(inp[k])[pad] != 0)]


def kind(name: str) -> str:
    """an output's name without the chunk number: gW1.part3 -> gW1.part.  The key of RESTATEMENT_RATIO / LAMBDA and of the GPU test's
    printed "mlp dqn layer ratios" line."""
    return re.sub(r"part\d+$", "part", name)


def failures(ops: dict, ex: dict, dev: dict, lam: Optional[dict] = None) -> list:
    lam = LAMBDA if lam is None else lam
    v = [check(ops[k], dev[k], lam[kind(k)]) for k in ops]
    return [x.message for x in v if not x.ok] + exact_failures(ex, dev)


def ratios(ops: dict, dev: dict) -> dict:
    return kind_ratios(ops, dev, by=kind)


# Criterion (c)'s factor per output: max(1, 4 x the largest |err| / (sqrt(n) u S) that the sequential float32 restatement reaches against
# f64 on the host inputs of every case (every batch of a case, both forms of a one-workgroup case).  `python tests/mlp_dqn_layer_reference.py`
# prints the table; tests/test_mlp_dqn_layer_reference.py recomputes all of it.  The 4 is for the device's accumulation order (k in
# MFMA groups of two lane halves, four k-slices summed through LDS, row chunks, the interleaved sums of the reduce) - it is NOT
# fitted to the device.
RESTATEMENT_RATIO = {
    "dy0": 0.986, "dy1": 0.995, "dy2": 0.987, "dy3": 0.443, "dy4": 0.391,
    "dy5": 0.750, "dy6": 0.450, "dy7": 0.967, "gW0": 1.098, "gW0.part": 1.007,
    "gW0.sum": 0.698, "gW1": 1.000, "gW1.part": 1.000, "gW1.sum": 0.706, "gW2": 0.888,
    "gW2.part": 0.920, "gW2.sum": 0.643, "gW3": 0.723, "gW3.part": 1.114, "gW3.sum": 0.000,
    "gW4.part": 0.890, "gW4.sum": 0.000, "gW5.part": 0.491, "gW5.sum": 0.000, "gW6.part": 0.261,
    "gW6.sum": 0.000, "gW7.part": 0.276, "gW7.sum": 0.000, "gW8.part": 0.747, "gW8.sum": 0.000,
    "z0.h0": 1.122, "z0.h1": 0.587, "z0.h2": 0.356, "z0.h3": 0.346, "z0.h4": 0.172,
    "z0.h5": 0.191, "z0.h6": 0.117, "z0.h7": 0.316, "z0.h8": 0.145, "z1.h0": 1.113,
    "z1.h1": 0.479, "z1.h2": 0.380, "z1.h3": 0.192, "z1.h4": 0.128, "z1.h5": 0.156,
    "z1.h6": 0.172, "z1.h7": 0.315, "z1.h8": 0.125, "z2.h0": 0.939, "z2.h1": 0.363,
    "z2.h2": 0.117,
}
LAMBDA = {k: max(1.0, 4.0 * v) for k, v in RESTATEMENT_RATIO.items()}


# ------------------------------------------------------------------------------------------------ float32 restatement
def _seq_dw(x, dy, r0, r1, skip=None, twice=None, times=0):
    """dW and db of rows [r0, r1) in f32, rows in order, products exact; `skip` drops a row, `twice` adds a row `times` more times"""
    x64, dy64 = np.asarray(x, F32).astype(np.float64), np.asarray(dy, F32).astype(np.float64)
    gw, gb = np.zeros((x64.shape[1], dy64.shape[1]), F32), np.zeros(dy64.shape[1], F32)
    for m in list(range(r0, r1)) + ([twice] * times if twice is not None else []):
        if m == skip: continue
        gw = _acc(gw, x64[m][:, None] * dy64[m][None, :]); gb = _acc(gb, dy64[m])
    return np.concatenate([gw.ravel(), gb])


MUTANTS = ("drop_dw_row", "drop_reduce_chunk", "stale_chunk", "alias_ragged_row", "target_through_online", "skip_k_slice", "tie_to_higher",
           "mask_ge_zero", "selector_from_target", "keep_clamped_gradient", "adam_skips_vector")


def restatement(inp: dict, mut: Optional[str] = None) -> dict:
    """device(inp) with every GEMM output replaced by its sequential-f32 evaluation from the same inputs and every row output by its
    restatement.  mut: one of MUTANTS - the wrong kernel of the host self-test."""
    c, B = inp["case"], inp["B"]
    lay = layers(c); L = c.L
    P, PT = arena(c, inp["q0"]), arena(c, inp["qt0"])
    out = {k: np.array(v, F32) for k, v in device(inp).items()}
    for z in range(c.nz):
        h = inp["x_in"][z]
        for l in range(L):
            W, b = (P if (z != 1 or mut == "target_through_online") else PT)[l]
            if mut == "skip_k_slice" and z == 0 and lay[l][2] >= 128:   # one wave's quarter of the reduction never added
                W = np.array(W); W[lay[l][2] // 4:lay[l][2] // 2] = 0
            v = _seq_mm(h, W, b)
            out["z%d.h%d" % (z, l)] = np.maximum(v, F32(0)) if lay[l][4] else v
            h = inp["acts"][z][l]
    for l in range(L - 2, -1, -1):
        v = _seq_mm(inp["dy"][l + 1], P[l + 1][0].T)
        a_ = np.asarray(inp["acts"][0][l])
        out["dy%d" % l] = np.where((a_ >= 0) if mut == "mask_ge_zero" else (a_ > 0), v, F32(0))
    xs = [inp["x_in"][0]] + list(inp["acts"][0][:L - 1])
    alias = dict(twice=B - 1, times=(-B) % 32) if mut == "alias_ragged_row" else {}
    for l in range(L):
        if inp["chunks"]:
            rows = dw_rows(B, inp["chunks"])
            for k, (r0, r1) in enumerate(rows):
                last = r1 == B and r1 > r0
                out["gW%d.part%d" % (l, k)] = _seq_dw(xs[l], inp["dy"][l], r0, r1, skip=(B - 1) if mut == "drop_dw_row" and last else None,
                                                      **(alias if last else {}))
            part = np.asarray(inp["part"][l], F32)
            acc = np.zeros(part.shape[1], F32)
            for k in range(part.shape[0]):
                if mut == "drop_reduce_chunk" and k == part.shape[0] - 1 and k > 0: continue
                acc = _acc(acc, part[k].astype(np.float64))
            if mut == "stale_chunk" and inp["chunks"] < predict_chunks(c, c.capacity, inp["form"]):
                acc = _acc(acc, np.asarray(inp.get("stale", inp["part"])[l], F32)[0].astype(np.float64))   # a chunk of an earlier, larger batch
            out["gW%d.sum" % l] = acc
        else:
            out["gW%d" % l] = _seq_dw(xs[l], inp["dy"][l], 0, B, skip=(B - 1) if mut == "drop_dw_row" else None, **alias)
    ex = exact(inp, mut)
    for k, cands in ex.items(): out[k] = np.array(cands[0], F32)
    return out


def all_host_inputs():
    """(label, inp) of every case, every batch, and for a one-workgroup case both forms"""
    for c in CASES.values():
        for env in ((), (("BDR_NO_MLP_LDS", "1"),)) if c.one_wg else ((),):
            for step in range(len(c.batches)):
                yield "%s%s[%d]" % (c.name, "/global" if env else "", c.batches[step]), host_inputs(c, step, env=env)


if __name__ == "__main__":   # the restatement's ratios on the host inputs of every case: sets RESTATEMENT_RATIO
    worst = {}
    for label, inp in all_host_inputs():
        r = ratios(reference(inp), restatement(inp))
        print(label, inp["form"], " ".join("%s %.3f" % kv for kv in sorted(r.items())), flush=True)
        for k, v in r.items(): worst[k] = max(worst.get(k, 0.0), v)
    print("RESTATEMENT_RATIO = {\n" + table_text(worst) + "\n}")
