"""Crafted inputs for the loss kernels' clamp, kink and saturation branches, and a float64 reference of every update they end.

Three pieces, used by tests/test_edge_inputs.py (CPU) and tests/test_gpu_loss_edges.py (GPU):

  dial networks   dial_mlp(): flat parameters (reference layout) of an Mlp whose output j is exactly one input column: first layer
                  h[2j] = relu(x_c), h[2j+1] = relu(-x_c), identity on those units through any further hidden layer, last layer
                  gain * (h[2j] - h[2j+1]) + bias.  Every sum has one non-zero term, so with gain a power of two and bias 0 the output is
                  x_c bit for bit in f32 in any summation order.  With rng given the other hidden units get random incoming weights
                  (their outgoing weights stay 0: the output is untouched, the last layer's weight gradient becomes dense).
  float64 refs    IqlRef / AwacRef / BcRef / SacRef / DqnRef / IqnRef: compact float64 autograd versions of the committed f32 code, the reference's
                  definitions kept (closed clamp ranges, the Jacobian on `a`, the f32 values of the configuration's constants), with
                  named mutations (`mut`) that restate plausible wrong kernels for the teeth test.
  case tables     CASES[agent]: named cases, each with the branch it targets, a coverage condition computed from the float64
                  reference alone, and the mutations it must catch.

Bars (checks_for): where the inputs of an element-wise stage are exact the bar is derived (a few ulp of f32 expf / logf / tanhf times the
conditioning, written beside the quantity); for sums over the batch it is 4 x the distance of the committed f32 restatement from
float64 on the same case, at most the ceiling of the agent's own GPU test file and at least n 2^-24 of the sum's largest term.
Nothing under border_amd/ imports this file.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass, field
from typing import Callable, Sequence

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):   # the restatements beside this file; oracle/ in the repository root
    if _p not in sys.path:
        sys.path.insert(0, _p)
import awac_restatement as RA  # noqa: E402
import bc_restatement as RB  # noqa: E402
import iql_restatement as RI  # noqa: E402
from oracle import torch_ref as T  # noqa: E402

DT = torch.float64
ULP = 2.0 ** -23          # one unit in the last place of an f32 in [1, 2): the relative spacing of f32
TINY = 2.0 ** -126        # the smallest normal f32: below it expf may return a subnormal or 0
CLAMP1 = float(np.float32(0.999999))   # the reference clamps f32 tensors: the constant is its f32 value, 1 - 17 * 2^-24


def f32(v) -> float:
    """the f32 value of a configuration constant (the reference's tensors are f32: 0.7 is 0.699999988...)"""
    return float(np.float32(v))


# ======================================================================================================== dial networks
def dial_mlp(in_dim: int, units: Sequence[int], out_dim: int, cols: Sequence, gain: float = 1.0, bias=None, rng=None) -> np.ndarray:
    """Flat f32 parameters (per layer weight [out][in] then bias [out]) of an Mlp with output j = gain * x[cols[j]] + bias[j].  An entry
    of cols may be a list of (column, gain) terms: output j is their sum, one pair of hidden units per term (exact where at most one
    term of a row is non-zero)."""
    terms = [[(c, gain)] if np.isscalar(c) else list(c) for c in cols]
    used = 2 * sum(len(t) for t in terms)
    assert len(cols) == out_dim and all(u >= used for u in units)
    dims = [in_dim] + list(units) + [out_dim]
    out = []
    for k in range(len(dims) - 1):
        o, i = dims[k + 1], dims[k]
        W, b = np.zeros((o, i), np.float64), np.zeros(o, np.float64)
        last, first = k == len(dims) - 2, k == 0
        if rng is not None and not last:   # the free hidden units: random incoming weights, no outgoing ones
            bd = 1.0 / math.sqrt(i)
            W[used:] = rng.uniform(-bd, bd, (o - used, i))
            b[used:] = rng.uniform(-bd, bd, o - used)
        u = 0
        for j, t in enumerate(terms):
            for c, g in t:
                if first and last:
                    W[j, c] = g
                elif first:
                    W[u, c], W[u + 1, c] = 1.0, -1.0
                elif last:
                    W[j, u], W[j, u + 1] = g, -g
                else:
                    W[u, u] = W[u + 1, u + 1] = 1.0
                u += 2
        if last and bias is not None:
            b[:] = bias
        out += [W.reshape(-1), b]
    return np.concatenate(out).astype(np.float32)


def const_mlp(in_dim, units, out_dim, hidden_bias: float, out_bias) -> np.ndarray:
    """all weights 0: every hidden unit is relu(hidden_bias), the output is out_bias"""
    dims = [in_dim] + list(units) + [out_dim]
    out = []
    for k in range(len(dims) - 1):
        o, i = dims[k + 1], dims[k]
        b = np.full(o, hidden_bias, np.float64)
        if k == len(dims) - 2:
            b[:] = out_bias
        out += [np.zeros(o * i), b]
    return np.concatenate(out).astype(np.float32)


def layer_slices(in_dim, units, out_dim):
    """[(weight slice, bias slice)] of each layer in the flat reference layout"""
    o, out = 0, []
    for (wo, wi), _ in RI.mlp_shapes(in_dim, units, out_dim):
        out.append((slice(o, o + wo * wi), slice(o + wo * wi, o + wo * wi + wo)))
        o += wo * wi + wo
    return out


# ======================================================================================================== float64 pieces
def relu_grad1_at_0(x):
    """mutation relu'(0) = 1: the same values, the gradient passes where x == 0"""
    return torch.where(x >= 0, x, torch.zeros_like(x))


class Net:
    """Mlp (mlp.rs:14-24) in `dtype`; mut "relu0": relu'(0) = 1 in the hidden layers and the output ReLU"""

    def __init__(self, in_dim, units, out_dim, relu_out, flat, dtype=DT):
        self.relu_out, self.params, o = relu_out, [], 0
        for ws, bs in RI.mlp_shapes(in_dim, units, out_dim):
            for s in (ws, bs):
                n = int(np.prod(s))
                self.params.append(torch.tensor(np.asarray(flat[o:o + n], np.float32).reshape(s), dtype=dtype, requires_grad=True))
                o += n
        assert o == len(flat), (o, len(flat))

    def __call__(self, x, mut=()):
        relu = relu_grad1_at_0 if "relu0" in mut else torch.relu
        n = len(self.params) // 2
        for k in range(n):
            x = x @ self.params[2 * k].T + self.params[2 * k + 1]
            if k < n - 1 or self.relu_out:
                x = relu(x)
        return x

    def flat(self, grad=False) -> np.ndarray:
        return np.concatenate([(p.grad if grad else p).detach().numpy().reshape(-1) for p in self.params]).astype(np.float64)

    def zero_grad(self):
        for p in self.params:
            p.grad = None


def row_terms(lvec, params, entries=False):
    """max over the batch rows of |d lvec_b / d theta| per parameter tensor: the largest term of each gradient sum"""
    n = lvec.shape[0]
    gs = torch.autograd.grad(lvec, params, grad_outputs=torch.eye(n, dtype=lvec.dtype), is_grads_batched=True, retain_graph=True,
                             allow_unused=True)
    if entries:   # also, per entry, the largest |term| of its sum (flat, in the arena's order)
        return ([0.0 if g is None else float(g.abs().max()) for g in gs],
                np.concatenate([np.zeros(p.numel()) if g is None else g.abs().amax(0).reshape(-1).numpy() for g, p in zip(gs, params)]))
    return [0.0 if g is None else float(g.abs().max()) for g in gs]


def smooth_l1_rows(p, t, mut=()):
    d = (p - t).abs()
    if "huber_quadratic" in mut:
        return 0.5 * d ** 2
    if "huber_linear" in mut:
        return d - 0.5
    return torch.where(d < 1.0, 0.5 * d ** 2, d - 0.5)


def adv_weights(s, adv, mut=()):
    """w = clamp(exp(inv_lambda adv), 0, exp_adv_max) | softmax over the batch (iql/base.rs:133-141, awac/base.rs:146-153)"""
    z = adv * f32(s.inv_lambda)
    if s.adv_softmax:
        if "softmax_no_max" in mut:   # exp(z) / sum(exp(z)) evaluated in f32: overflows where z > 88.7
            e = z.to(torch.float32).exp()
            return (e / e.sum()).to(z.dtype)
        return torch.softmax(z, 0)
    if "w_clamp_dropped" in mut:
        return z.exp()
    return z.exp().clamp(0.0, f32(s.exp_adv_max))


def gauss_logp(s, mean, head2, act, mut=()):
    """GaussianActor::logp (util/actor.rs:196-223): std = exp(clamp(head2, min, max)); Tanh limit: x = atanh(clamp(a / scale)) and the
    log-Jacobian of the action itself (util.rs:268-279)"""
    lo, hi = f32(s.min_log_std), f32(s.max_log_std)
    h = head2.expand(act.shape[0], -1)
    c = h.clamp(lo, hi)
    if "lstd_clamp_dropped" in mut:
        c = h
    elif "lstd_grad_open" in mut:          # the clamped value, the gradient of the identity
        c = h + (c - h).detach()
    elif "lstd_grad_half_open" in mut:     # min < h <= max
        c = c.detach() + (h - h.detach()) * ((h > lo) & (h <= hi)).to(h.dtype)
    elif "lstd_grad_open_interval" in mut:  # min < h < max
        c = c.detach() + (h - h.detach()) * ((h > lo) & (h < hi)).to(h.dtype)
    std = c.exp()
    var = std ** 2
    nlp = lambda x: (-0.5 * math.log(2 * math.pi) - 0.5 * var.log() - (0.5 / var) * (x - mean) ** 2).sum(-1)
    if s.action_limit == "Clamp":
        return nlp(act.clamp(f32(s.action_min), f32(s.action_max)) if "logp_clamps_act" in mut else act)
    t = act / f32(s.action_scale)
    if "atanh_clamp_dropped" not in mut:
        t = t.clamp(-CLAMP1, CLAMP1)
    x = 0.5 * ((1.0 + t) / (1.0 - t)).log()
    a = act / f32(s.action_scale) if "jac_on_scaled" in mut else act
    if "jac_clamp_dropped" not in mut:
        a = a.clamp(-CLAMP1, CLAMP1)
    return nlp(x) + (-1.0 * (1.0 - a ** 2).log()).sum(-1)


def policy_sample(s, actor, head2, obs, z, mut=()):
    """Policy::sample (util/actor.rs:226-241): z None = eval mode (the mean)"""
    with torch.no_grad():
        mean = actor(obs)
        std = head2.clamp(f32(s.min_log_std), f32(s.max_log_std)).exp()
        if "sample_lstd_clamp_dropped" in mut:
            std = head2.exp()
        a = mean if z is None else std * z + mean
        if s.action_limit == "Clamp":
            return a if "sample_clamp_dropped" in mut else a.clamp(f32(s.action_min), f32(s.action_max))
        return f32(s.action_scale) * a.tanh()


def _gnd(s, term, trunc, mut, dtype):
    term, trunc = np.asarray(term, np.int8), np.asarray(trunc, np.int8)
    done = term if "trunc_ignored" in mut else (term | trunc)
    if "done_ignored" in mut:
        done = 0 * term
    return torch.as_tensor((1.0 - done.astype(np.float64)) * f32(s.gamma), dtype=dtype)


def _opt(s, name, params, lr):
    kw = s.adamw.get(name)
    return RI.AdamState(params, lr, adamw=kw is not None, **(kw or {}))


# ======================================================================================================== IQL
class IqlRef:
    """Iql::opt_ (iql/base.rs:157-188) in float64; update() returns every compared quantity in one dict"""

    def __init__(self, spec, actor, critics, critics_tgt, value, mut=(), dtype=DT):
        s = self.spec = spec
        self.mut, self.dtype = frozenset(mut), dtype
        O, A = s.obs_dim, s.act_dim
        self.actor = Net(O, s.p_units, A, False, actor[:-A], dtype)
        self.head2 = torch.tensor(np.asarray(actor[-A:], np.float32).reshape(1, A), dtype=dtype, requires_grad=True)
        self.critics = [Net(O + A, s.q_units, 1, s.q_relu_out, c, dtype) for c in critics]
        self.targets = [Net(O + A, s.q_units, 1, s.q_relu_out, c, dtype) for c in critics_tgt]
        self.value = Net(O, s.v_units, 1, s.v_relu_out, value, dtype)
        self.opt_v = _opt(s, "value", self.value.params, s.lr_value)
        self.opt_q = _opt(s, "critic", [p for c in self.critics for p in c.params], s.lr_critic)
        self.opt_pi = _opt(s, "actor", self.actor.params + [self.head2], s.lr_actor)

    def q_tgt_min(self, x):
        with torch.no_grad():
            return torch.stack([t(x).squeeze(-1) for t in self.targets], 0).min(0).values

    def update(self, obs, act, next_obs, reward, term, trunc, terms=False) -> dict:
        s, mut = self.spec, self.mut
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32), dtype=self.dtype)
        obs, act, next_obs, reward = t(obs), t(act), t(next_obs), t(reward).reshape(-1)
        n = obs.shape[0]
        gnd = _gnd(s, term, trunc, mut, self.dtype)
        out, tm = {}, {}
        x = torch.cat([obs, act], 1)
        # update_value
        self.value.zero_grad()
        q = self.q_tgt_min(x)
        v = self.value(obs, mut).squeeze(-1)
        u = q - v
        neg = (u > 0) if "expectile_flipped" in mut else (u < 0)
        wt = torch.full_like(u, 0.5) if "expectile_dropped" in mut else (f32(s.tau_iql) - neg.to(u.dtype)).abs()
        lv = wt * u ** 2 / n
        if terms:
            tm["grad_value"] = row_terms(lv, self.value.params)
        lv.sum().backward()
        out.update(q_tgt_min_value=q, v=v, u=u, loss_value=lv.sum(), grad_value=self.value.flat(True), terms_loss_value=lv)
        self.opt_v.step()
        # update_critic
        for c in self.critics:
            c.zero_grad()
        preds = [c(x, mut).squeeze(-1) for c in self.critics]
        with torch.no_grad():
            v_next = self.value(next_obs).squeeze(-1)
            tgt = reward + gnd * v_next
        nc = len(preds)
        rows = [(((p - tgt) ** 2) if s.critic_loss == "Mse" else smooth_l1_rows(p, tgt, mut)) / (n * nc) for p in preds]
        if terms:
            for i, c in enumerate(self.critics):
                tm[f"grad_critic_{i}"] = row_terms(rows[i], c.params)
        lq = torch.stack(rows, 0)
        lq.sum().backward()
        out.update(tgt=tgt, v_next=v_next, q_pred=torch.stack(preds), loss_critic=lq.sum(), terms_loss_critic=lq.reshape(-1))
        for i, c in enumerate(self.critics):
            out[f"grad_critic_{i}"] = c.flat(True)
        self.opt_q.step()
        with torch.no_grad():
            for c, tc in zip(self.critics, self.targets):
                for p, tp in zip(c.params, tc.params):
                    tp.copy_(f32(s.critic_tau) * p + (1.0 - f32(s.critic_tau)) * tp)
        # update_actor
        self.actor.zero_grad(); self.head2.grad = None
        q3 = self.q_tgt_min(x)
        with torch.no_grad():
            v_obs = self.value(obs).squeeze(-1)
            w = adv_weights(s, q3 - v_obs, mut)
        mean = self.actor(obs, mut)
        logp = gauss_logp(s, mean, self.head2, act, mut)
        la = -1.0 * logp * w / n
        if terms:
            tm["grad_actor"] = row_terms(la, self.actor.params + [self.head2])
            out["addends_loss_actor"] = logp_addend_max(s, mean.detach().numpy(), self.head2.detach().numpy(), act.numpy()) * w.numpy() / n
            out["n_act"] = s.act_dim
        la.sum().backward()
        out.update(q_tgt_min_actor=q3, v_obs=v_obs, w=w, logp=logp, loss_actor=la.sum(), terms_loss_actor=la,
                   grad_actor=np.concatenate([self.actor.flat(True), self.head2.grad.numpy().reshape(-1)]))
        self.opt_pi.step()
        out.update(param_actor=np.concatenate([self.actor.flat(), self.head2.detach().numpy().reshape(-1)]), param_value=self.value.flat())
        for i in range(nc):
            out[f"param_critic_{i}"] = self.critics[i].flat()
            out[f"param_critic_tgt_{i}"] = self.targets[i].flat()
        out = {k: (v.detach().numpy().astype(np.float64) if torch.is_tensor(v) else v) for k, v in out.items()}
        out["row_terms"] = tm
        return out


def iql_f32(spec, params, batches) -> dict:
    """the committed f32 restatement on the same case, under IqlRef's keys (the last update's quantities)"""
    r = RI.IqlRestatement(spec, *params)
    for b in batches:
        rec = r.update(*b)
    p = r.probes
    out = {k: p[k] for k in ("q_tgt_min_value", "v", "u", "tgt", "v_next", "q_pred", "q_tgt_min_actor", "v_obs", "w", "logp")}
    out.update(rec, grad_value=p["value_grad"], grad_actor=p["actor_grad"], param_actor=r.params("actor"), param_value=r.params("value"))
    for i in range(spec.n_critics):
        out[f"grad_critic_{i}"] = p["critic_grads"][i]
        out[f"param_critic_{i}"], out[f"param_critic_tgt_{i}"] = r.params(f"critic_{i}"), r.params(f"critic_tgt_{i}")
    return out


# ======================================================================================================== AWAC
class AwacRef:
    """Awac::opt_ (awac/base.rs:170-215) in float64"""

    def __init__(self, spec, actor, critics, critics_tgt, mut=(), dtype=DT):
        s = self.spec = spec
        self.mut, self.dtype = frozenset(mut), dtype
        O, A = s.obs_dim, s.act_dim
        self.actor = Net(O, s.p_units, A, False, actor[:-A], dtype)
        self.head2 = torch.tensor(np.asarray(actor[-A:], np.float32).reshape(1, A), dtype=dtype, requires_grad=True)
        self.critics = [Net(O + A, s.q_units, 1, s.q_relu_out, c, dtype) for c in critics]
        self.targets = [Net(O + A, s.q_units, 1, s.q_relu_out, c, dtype) for c in critics_tgt]
        self.opt_q = _opt(s, "critic", [p for c in self.critics for p in c.params], s.lr_critic)
        self.opt_pi = _opt(s, "actor", self.actor.params + [self.head2], s.lr_actor)

    @staticmethod
    def q_min(nets, obs, act):
        x = torch.cat([obs, act], 1)
        with torch.no_grad():
            return torch.stack([n(x).squeeze(-1) for n in nets], 0).min(0).values

    def update(self, obs, act, next_obs, reward, term, trunc, z_pi=None, z_next=None, terms=False) -> dict:
        s, mut = self.spec, self.mut
        t = lambda x: None if x is None else torch.as_tensor(np.asarray(x, np.float32), dtype=self.dtype)
        obs, act, next_obs, reward, z_pi, z_next = t(obs), t(act), t(next_obs), t(reward).reshape(-1), t(z_pi), t(z_next)
        n = obs.shape[0]
        gnd = _gnd(s, term, trunc, mut, self.dtype)
        out, tm = {}, {}
        # update_actor
        self.actor.zero_grad(); self.head2.grad = None
        act_ = policy_sample(s, self.actor, self.head2, obs, z_pi, mut)
        q = self.q_min(self.critics, obs, act)
        v = self.q_min(self.targets if "v_from_targets" in mut else self.critics, obs, act_)
        adv = q - v
        with torch.no_grad():
            w = adv_weights(s, adv, mut)
        mean = self.actor(obs, mut)
        logp = gauss_logp(s, mean, self.head2, act, mut)
        la = -1.0 * logp * w / n
        if terms:
            tm["grad_actor"] = row_terms(la, self.actor.params + [self.head2])
            out["addends_loss_actor"] = logp_addend_max(s, mean.detach().numpy(), self.head2.detach().numpy(), act.numpy()) * w.numpy() / n
            out["n_act"] = s.act_dim
        la.sum().backward()
        out.update(q_data_min=q, q_pi_min=v, adv=adv, w=w, logp=logp, act_=act_, loss_actor=la.sum(), terms_loss_actor=la,
                   adv_mean=adv.mean(), adv_abs_mean=adv.abs().mean(), logp_mean=logp.mean(),
                   grad_actor=np.concatenate([self.actor.flat(True), self.head2.grad.numpy().reshape(-1)]))
        self.opt_pi.step()
        # update_critic, next_act from the actor just updated
        for c in self.critics:
            c.zero_grad()
        x = torch.cat([obs, act], 1)
        preds = [c(x, mut).squeeze(-1) for c in self.critics]
        next_act = policy_sample(s, self.actor, self.head2, next_obs, z_next, mut)
        next_q = self.q_min(self.targets, next_obs, next_act)
        tgt = reward + gnd * next_q
        rows = [(((p - tgt) ** 2) if s.critic_loss == "Mse" else smooth_l1_rows(p, tgt, mut)) / n for p in preds]   # SUM over the critics
        if terms:
            for i, c in enumerate(self.critics):
                tm[f"grad_critic_{i}"] = row_terms(rows[i], c.params)
        lq = torch.stack(rows, 0)
        lq.sum().backward()
        out.update(next_act=next_act, next_q=next_q, tgt=tgt, q_pred=torch.stack(preds), loss_critic=lq.sum(), terms_loss_critic=lq.reshape(-1),
                   q_tgt_abs_mean=tgt.abs().mean(), reward_mean=reward.mean(), next_q_mean=next_q.mean())
        for i, c in enumerate(self.critics):
            out[f"grad_critic_{i}"] = c.flat(True)
        self.opt_q.step()
        with torch.no_grad():
            for c, tc in zip(self.critics, self.targets):
                for p, tp in zip(c.params, tc.params):
                    tp.copy_(f32(s.critic_tau) * p + (1.0 - f32(s.critic_tau)) * tp)
        out.update(param_actor=np.concatenate([self.actor.flat(), self.head2.detach().numpy().reshape(-1)]))
        for i in range(len(preds)):
            out[f"param_critic_{i}"] = self.critics[i].flat()
            out[f"param_critic_tgt_{i}"] = self.targets[i].flat()
        out = {k: (v.detach().numpy().astype(np.float64) if torch.is_tensor(v) else v) for k, v in out.items()}
        out["row_terms"] = tm
        return out


def awac_f32(spec, params, batches) -> dict:
    r = RA.AwacRestatement(spec, *params)
    for b in batches:
        rec = r.update(*b)
    p = r.probes
    out = {k: p[k] for k in ("q_data_min", "q_pi_min", "adv", "w", "logp", "act_", "next_act", "next_q", "tgt", "q_pred")}
    out.update(rec, grad_actor=p["actor_grad"], param_actor=r.params("actor"))
    for i in range(spec.n_critics):
        out[f"grad_critic_{i}"] = p["critic_grads"][i]
        out[f"param_critic_{i}"], out[f"param_critic_tgt_{i}"] = r.params(f"critic_{i}"), r.params(f"critic_tgt_{i}")
    return out


# ======================================================================================================== BC
def _sigmoid_e_over_1pe_f32(z):
    e = z.detach().to(torch.float32).exp()
    return (e / (1.0 + e)).to(z.dtype) + (torch.sigmoid(z) - torch.sigmoid(z).detach())   # f32 e / (1 + e) values, the true gradient


class BcRef:
    """Bc::opt_ (bc/base.rs:167-198) in float64"""

    def __init__(self, spec, flat, mut=(), dtype=DT):
        self.spec, self.mut, self.dtype = spec, frozenset(mut), dtype
        self.net = Net(spec.obs_dim, spec.units, spec.act_dim, False, flat, dtype)
        self.opt = RI.AdamState(self.net.params, spec.lr, adamw=spec.adamw is not None, **(spec.adamw or {}))

    def act_out(self, z):
        kind, mut = self.spec.activation_out, self.mut
        if kind == "ReLU":
            return relu_grad1_at_0(z) if "relu0" in mut else torch.relu(z)
        if kind == "Tanh":
            if "tanh_grad_of_z" in mut:        # 1 - z^2 for 1 - tanh(z)^2: right to second order at 0
                return torch.tanh(z).detach() + (z - z ** 3 / 3 - (z - z ** 3 / 3).detach())
            return torch.tanh(z)
        if kind == "Sigmoid":
            if "sigmoid_e_over_1pe" in mut:
                return _sigmoid_e_over_1pe_f32(z)
            if "sigmoid_grad_y" in mut:        # y for y (1 - y)
                y = torch.sigmoid(z)
                return y.detach() + (z - z.detach()) * y.detach()
            return torch.sigmoid(z)
        return z

    def update(self, obs, act, terms=False) -> dict:
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32), dtype=self.dtype)
        obs, act = t(obs), t(act)
        self.net.zero_grad()
        z = self.net(obs, self.mut)
        pred = self.act_out(z)
        d = pred - act
        if "out_act_dropped" in self.mut:
            d = z - act
        lrow = (d * d).sum(-1) / d.numel()
        tm = {"grad": row_terms(lrow, self.net.params)} if terms else {}
        dz, = torch.autograd.grad(lrow.sum(), z, retain_graph=True)
        lrow.sum().backward()
        out = dict(pred=pred.detach().numpy().copy(), dz=dz.numpy().copy(), loss=float(lrow.sum().detach()), grad=self.net.flat(True),
                   terms_loss=(d * d).detach().numpy().reshape(-1) / d.numel(), z=z.detach().numpy().copy())
        self.opt.step()
        out.update(param=self.net.flat(), row_terms=tm)
        return out


def bc_f32(spec, params, batches) -> dict:
    r = RB.BcRestatement(spec, *params)
    for b in batches:
        rec = r.update(*b)
    return dict(pred=r.probes["pred"], dz=r.probes["dz"], grad=r.probes["grad"], loss=rec["loss"], param=r.params())


# ======================================================================================================== cases, bars, checks
@dataclass
class Case:
    name: str
    agent: str
    spec: object
    params: tuple                      # initial parameters, the agent's set_params order
    batches: list                      # one tuple of update_on_batch arguments per step
    branch: str                        # the branch of the loss kernel this case is there for
    coverage: Callable                 # float64 output of the last step -> {side: (count, total, on_boundary)}
    muts: tuple                        # mutations of the reference that this case must catch
    exact: tuple = ()                  # keys that the construction makes exact: compared bit for bit
    derived: dict = field(default_factory=dict)   # key -> callable(ref) -> (rel, abs): |got - ref| <= rel |ref| + abs element by element
    zero: dict = field(default_factory=dict)      # key -> index array: entries that must be == 0
    build: dict = field(default_factory=dict)     # keywords of the agent's to_config
    random_units: str = ""             # which networks keep random weights in their free units


def covered(cov: dict) -> list:
    """the sides that miss the condition fixed in advance: 20 % of the rows, or 2 rows for a side placed exactly on a boundary"""
    return [k for k, (c, n, edge) in cov.items() if (c < 2 if edge else c < 0.2 * n)]


def run_ref(case: Case, mut=(), terms=False, dtype=DT) -> dict:
    """the float64 reference (or a mutation of it) over the case's steps; the last step's quantities"""
    cls = {"iql": IqlRef, "awac": AwacRef, "bc": BcRef, "sac": SacRef, "dqn": DqnRef, "iqn": IqnRef}[case.agent]
    mut = tuple(x for m in mut for x in m.split("+"))   # "a+b": two mutations at once
    r = cls(case.spec, *case.params, mut=mut, dtype=dtype)
    for k, b in enumerate(case.batches):
        out = r.update(*b, terms=terms and k == len(case.batches) - 1)
    return out


def run_f32(case: Case) -> dict:
    return {"iql": iql_f32, "awac": awac_f32, "bc": bc_f32, "sac": sac_f32, "dqn": dqn_f32, "iqn": iqn_f32}[case.agent](case.spec, case.params, case.batches)


def relmax(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not np.isfinite(a).all():
        return math.inf
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@dataclass
class Check:
    key: str            # the quantity (a key of the reference's output)
    kind: str           # exact | elem | rel | abs | zero
    bar: object = 0.0   # rel / abs: the bar; elem: (rel, abs)
    sl: object = None   # a slice or index array of the flattened quantity
    how: str = ""       # where the bar comes from
    against: str = "f64"   # parameters and targets keep their existing reference, the f32 restatement (the Adam step is under test in
                           # tests/optimizer_inputs.py, element by element from the device's own gradient, not here: on gradients of
                           # 1e-20 an f32 and a float64 Adam of the WHOLE update legitimately differ by more than 0.3 lr)

    def _pick(self, x):
        x = np.asarray(x, np.float64).reshape(-1)
        return x if self.sl is None else x[self.sl]

    def err(self, got, ref) -> float:
        g, r = self._pick(got[self.key]), self._pick(ref[self.key])
        if not np.isfinite(g).all():
            return math.inf
        if self.kind == "zero":
            return float(np.abs(g).max()) if g.size else 0.0
        if self.kind in ("exact", "abs"):
            return float(np.abs(g - r).max())
        if self.kind == "rel":
            return relmax(g, r)
        rel, ab = (np.asarray(x, np.float64).reshape(-1) if np.ndim(x) else x for x in self.bar)
        return float((np.abs(g - r) / (rel * np.abs(r) + ab)).max())   # elem: already in units of the bar

    def ratio(self, got, ref) -> float:
        """the error in units of the bar: <= 1 passes; the teeth test asks a mutation for >= 10 somewhere"""
        e = self.err(got, ref)
        if self.kind == "elem":
            return e
        if self.kind in ("exact", "zero") or self.bar == 0.0:
            return 0.0 if e == 0.0 else math.inf
        return e / self.bar


def sum_bar(dist: float, floor: float, ceiling: float) -> float:
    """a sum over the batch against float64: 4 x the committed f32 restatement's distance (two f32 implementations that sum in different
    orders), at most the ceiling of the agent's GPU test file, at least n 2^-24 of the largest term"""
    return min(ceiling, max(4.0 * dist, floor))


def _loss_check(key, ref, f32out, terms_key):
    t = np.abs(ref[terms_key])
    floor = t.size * 2.0 ** -24 * float(t.max())
    if key == "loss_actor" and "addends_loss_actor" in ref:
        # the kernel adds w_b / n times (c - log std_j), q_bj and log(1 - a_bj^2) over rows AND action columns, all in f32; a row's logp hides
        # the cancellation among them (q_bj reaches 1e5 where log std is clamped at -5).  The sum's terms are these addends: 3 A n of them.
        a = np.abs(ref["addends_loss_actor"])
        floor = a.size * 3 * ref["n_act"] * 2.0 ** -24 * float(a.max())
    dist = abs(float(f32out[key]) - float(ref[key]))
    ceil = 5e-4 * abs(float(ref[key])) + 1e-6
    return Check(key, "abs", sum_bar(dist, floor, ceil), how=f"f32 dist {dist:.3g} floor {floor:.3g} ceiling {ceil:.3g}")


def _sizes(shapes) -> list:
    """element counts of the parameter tensors, from mlp_shapes of either form ([(w, b), ...] or [w, b, ...])"""
    flat = [x for sh in shapes for x in (sh if isinstance(sh[0], tuple) else (sh,))]
    return [int(np.prod(x)) for x in flat]


def _grad_checks(key, ref, f32out, n_sum, tmax, last: slice, ceiling=2e-3, tail=None, sizes=()):
    """the arena as a whole and its last layer on its own scale (max-relative); every parameter tensor (sizes) whose reference gradient is
    exactly 0 - the hidden layers behind an all-zero layer - is asked for exact zeros"""
    out, o = [], 0
    g = np.asarray(ref[key]).reshape(-1)
    assert not sizes or sum(sizes) == g.size, (key, sum(sizes), g.size)
    for k, cnt in enumerate(sizes):
        if np.abs(g[o:o + cnt]).max() == 0.0:
            out.append(Check(key, "zero", sl=slice(o, o + cnt), how=f"the reference is exactly 0 in tensor {k}"))
        o += cnt
    for tag, sl, tm in (("", None, max(tmax)), (" last layer", last, max(tmax[-(tail or (3 if key == "grad_actor" else 2)):]))):
        r = np.asarray(ref[key]).reshape(-1)[sl if sl is not None else slice(None)]
        if np.abs(r).max() == 0.0:
            out.append(Check(key, "zero", sl=sl, how="the reference is exactly 0" + tag))
            continue
        f = np.asarray(f32out[key], np.float64).reshape(-1)[sl if sl is not None else slice(None)]
        dist = relmax(f, r)
        floor = n_sum * 2.0 ** -24 * tm / float(np.abs(r).max())
        out.append(Check(key, "rel", sum_bar(dist, floor, ceiling), sl=sl, how=f"f32 dist {dist:.3g} floor {floor:.3g} ceiling {ceiling:g}" + tag))
    return out


def _last_slice(in_dim, units, out_dim, extra=0):
    w, b = layer_slices(in_dim, units, out_dim)[-1]
    return slice(w.start, b.stop + extra)


def checks_for(case: Case, ref: dict, f32out: dict) -> list:
    """every comparison of the GPU test, in its order: exact probes, the other probes, losses, gradients, parameters and targets.
    ref must come from run_ref(case, terms=True)."""
    s, out = case.spec, []
    n = len(case.batches[-1][0])
    for k in case.exact:
        out.append(Check(k, "exact", how="exact by construction"))
    for k, sl in case.zero.items():
        out.append(Check(k, "zero", sl=sl, how="must be exactly 0"))
    for k, fn in case.derived.items():
        out.append(Check(k, "elem", fn(ref), how="derived from the f32 formats"))
    tm = ref["row_terms"]
    if case.agent in ("iql", "awac"):
        O, A = s.obs_dim, s.act_dim
        probes = {"iql": ("q_tgt_min_value", "v", "tgt", "v_next", "q_tgt_min_actor", "v_obs", "logp", "q_pred"),
                  "awac": ("q_data_min", "q_pi_min", "next_q", "tgt", "logp", "act_", "next_act", "q_pred")}[case.agent]
        for k in probes:   # the ceilings of _check_probes
            if np.abs(ref[k]).max() > 0:
                out.append(Check(k, "rel", 1e-4, how="ceiling (_check_probes)"))
            else:
                out.append(Check(k, "zero", how="the reference is exactly 0"))
        qk = "q_tgt_min_value" if case.agent == "iql" else "q_data_min"
        out.append(Check("u" if case.agent == "iql" else "adv", "abs", 1e-4 * float(np.abs(ref[qk]).max()) + 1e-6, how="ceiling (_check_probes)"))
        out.append(Check("w", "rel", 2e-3, how="ceiling (_check_probes)"))
        losses = ("loss_value", "loss_critic", "loss_actor") if case.agent == "iql" else ("loss_critic", "loss_actor")
        for k in losses:
            out.append(_loss_check(k, ref, f32out, "terms_" + k))
        if case.agent == "awac":
            for k, src in (("adv_mean", "adv"), ("adv_abs_mean", "adv"), ("logp_mean", "logp"), ("reward_mean", None), ("next_q_mean", "next_q"),
                           ("q_tgt_abs_mean", "tgt")):
                want = float(ref[k])
                ceil = (1e-4 * max(1.0, float(ref["q_tgt_abs_mean"])) + 5e-4 * abs(want)) if k.startswith("adv") else 5e-4 * abs(want) + 1e-6
                # These means are not losses; their bar is this file's own.  An f32 mean of n f32 terms, blocked or pairwise in any order:
                # each of the ceil(log2 n) levels rounds partial sums that add up to at most sum|x|, then 1 / n is rounded, the product
                # is rounded and the result is stored as f32: (ceil(log2 n) + 3) 2^-24 mean|x|; 4 x the f32 restatement's distance where
                # that is more, the ceiling of _check_rec where that is less.
                t = np.abs(ref[src]) if src else np.abs(np.asarray(case.batches[-1][3], np.float64))
                floor = (math.ceil(math.log2(n)) + 3) * 2.0 ** -24 * float(t.mean())
                out.append(Check(k, "abs", sum_bar(abs(float(f32out[k]) - want), floor, ceil), how=f"record mean: floor {floor:.3g} ceiling {ceil:.3g}"))
        nsum = n + max(max(s.p_units), max(s.q_units))
        out += _grad_checks("grad_actor", ref, f32out, nsum, tm["grad_actor"], _last_slice(O, s.p_units, A, A), sizes=_sizes(RI.mlp_shapes(O, s.p_units, A)) + [A])
        for i in range(s.n_critics):
            out += _grad_checks(f"grad_critic_{i}", ref, f32out, nsum, tm[f"grad_critic_{i}"], _last_slice(O + A, s.q_units, 1),
                                sizes=_sizes(RI.mlp_shapes(O + A, s.q_units, 1)))
        if case.agent == "iql":
            out += _grad_checks("grad_value", ref, f32out, n + max(s.v_units), tm["grad_value"], _last_slice(O, s.v_units, 1), sizes=_sizes(RI.mlp_shapes(O, s.v_units, 1)))
            out.append(Check("param_value", "abs", 0.3 * s.lr_value, how="ceiling (_check_state)"))
        out.append(Check("param_actor", "abs", 0.3 * s.lr_actor, how="ceiling (_check_state)"))
        for i in range(s.n_critics):
            out.append(Check(f"param_critic_{i}", "abs", 0.3 * s.lr_critic, how="ceiling (_check_state)"))
            out.append(Check(f"param_critic_tgt_{i}", "rel", 1e-5, how="ceiling (_check_state)"))
    elif case.agent == "sac":
        O, A = s.obs_dim, s.act_dim
        for k in ("q_pi", "q_pred", "q_next", "qvals_min", "tgt", "next_act", "log_p", "next_log_p"):   # QTOL of tests/test_gpu_sac.py
            out.append(Check(k, "rel", 1e-4, how="ceiling (QTOL)"))
        for k, rel_c in (("loss_critic", 1e-4), ("loss_actor", 5e-4)):
            c = _loss_check(k, ref, f32out, "terms_" + k)
            c.bar = min(c.bar, rel_c * abs(float(ref[k])) + 1e-6)
            out.append(c)
        want = float(ref["ent_coef"])
        out.append(Check("ent_coef", "abs", sum_bar(abs(float(f32out["ent_coef"]) - want), 4 * ULP * want, 5e-4 * want + 1e-6), how="alpha = exp(log_alpha)"))
        nsum = n + max(max(s.pi_units), max(s.q_units))
        w, b = layer_slices(O, s.pi_units, 2 * A)[-1]
        out += _grad_checks("grad_pi", ref, f32out, nsum, tm["grad_pi"], slice(w.start, b.stop), tail=4, sizes=_sizes(RI.mlp_shapes(O, s.pi_units, 2 * A)[:-1]) + [A * s.pi_units[-1], A] * 2)
        for i in range(s.n_critics):
            out += _grad_checks(f"grad_q_{i}", ref, f32out, nsum, tm[f"grad_q_{i}"], _last_slice(O + A, s.q_units, 1), sizes=_sizes(RI.mlp_shapes(O + A, s.q_units, 1)))
            out.append(Check(f"param_q_{i}", "abs", 0.3 * s.lr_critic, how="ceiling"))
            out.append(Check(f"param_q_tgt_{i}", "rel", 1e-5, how="ceiling"))
        out.append(Check("param_pi", "abs", 0.3 * s.lr_actor, how="ceiling"))
        out.append(Check("log_alpha", "abs", 1e-6, how="ceiling", against="f32"))
    elif case.agent == "dqn":
        for k in ("q_pred_all", "q_next_all", "pred", "tgt") + (("td_errs",) if "td_errs" in ref and len(case.batches[-1]) > 5 else ()):   # QTOL of tests/test_gpu_dqn.py
            out.append(Check(k, "rel", 1e-4, how="ceiling (QTOL)") if np.abs(ref[k]).max() > 0 else Check(k, "zero", how="the reference is exactly 0"))
        c = _loss_check("loss", ref, f32out, "terms_loss")
        c.bar = min(c.bar, 1e-4 * abs(float(ref["loss"])) + 1e-9)
        out.append(c)
        o, nsum = 0, n + (max(s.units) if s.kind == "mlp" else 3136)
        for sh, tmax in zip(s.shapes(), tm["grad"]):   # per variable, the ceiling of assert_grads_close with no flipped unit allowed
            cnt = int(np.prod(sh))
            sl = slice(o, o + cnt)
            o += cnt
            r = ref["grad"][sl]
            if np.abs(r).max() == 0.0:
                out.append(Check("grad", "zero", sl=sl, how=f"the reference is exactly 0 {sh}"))
                continue
            dist = relmax(np.asarray(f32out["grad"], np.float64)[sl], r)
            floor = nsum * 2.0 ** -24 * tmax / float(np.abs(r).max())
            out.append(Check("grad", "rel", sum_bar(dist, floor, 2e-4), sl=sl, how=f"f32 dist {dist:.3g} floor {floor:.3g} ceiling 2e-4 {sh}"))
        # Parameters after the first Adam step, lr g / (|g| + eps).  An entry none of whose rows contributes (dead units, the trunk behind a
        # zero head) has gradient exactly 0 and must not move: == its initial value.  An entry whose rows' terms are not 0 but cancel below
        # the floor of their own sum (n 2^-24 of the entry's largest term) has an f32 gradient whose sign is rounding noise, so two correct
        # steps can differ by 2 lr.  Every other entry keeps the 0.3 lr of tests/test_gpu_dqn.py.
        emax = tm["grad_entry_max"]
        dead = emax == 0.0
        cancel = ~dead & (np.abs(ref["grad"]) <= nsum * 2.0 ** -24 * emax)
        if dead.any():
            out.append(Check("param", "exact", sl=np.flatnonzero(dead), how=f"{int(dead.sum())} entries with no contributing row: unchanged", against="init"))
        out.append(Check("param", "elem", (0.0, np.where(cancel, 2.0 * s.lr, 0.3 * s.lr)),
                         how=f"ceiling 0.3 lr; 2 lr on the {int(cancel.sum())} of {cancel.size} entries whose non-zero terms cancel below their floor"))
        out.append(Check("param_tgt", "rel", 1e-3, how="ceiling"))
    elif case.agent == "iqn":
        c = _loss_check("loss_critic", ref, f32out, "terms_loss")
        c.bar = min(c.bar, 1e-4 * abs(float(ref["loss_critic"])) + 1e-9)     # QTOL of tests/test_gpu_iqn.py
        out.append(c)
        b0 = case.batches[-1]
        npairs = b0[5].shape[1] * b0[6].shape[1]
        o = 0
        for sh, tmax in zip(s.shapes(), tm["grad"]):   # per variable; the ceiling is the 5e-4 of tests/test_gpu_iqn.py
            cnt = int(np.prod(sh))
            sl = slice(o, o + cnt)
            o += cnt
            r = ref["grad"][sl]
            if np.abs(r).max() == 0.0:
                out.append(Check("grad", "zero", sl=sl, how=f"the reference is exactly 0 {sh}"))
                continue
            dist = relmax(np.asarray(f32out["grad"], np.float64)[sl], r)
            floor = (n * npairs + max(s.f_units)) * 2.0 ** -24 * tmax / npairs / float(np.abs(r).max())
            out.append(Check("grad", "rel", sum_bar(dist, floor, 5e-4), sl=sl, how=f"f32 dist {dist:.3g} floor {floor:.3g} ceiling 5e-4 {sh}"))
        out.append(Check("param", "abs", 0.1 * s.lr, how="ceiling"))
        out.append(Check("param_tgt", "rel", 1e-5, how="ceiling"))
    else:   # bc
        for k in ("pred", "dz"):
            if np.abs(ref[k]).max() > 0:
                out.append(Check(k, "rel", 1e-4, how="ceiling (_check_step)"))
        out.append(_loss_check("loss", ref, f32out, "terms_loss"))
        units = list(s.units)
        out += _grad_checks("grad", ref, f32out, n + (max(units) if units else 0), tm["grad"], _last_slice(s.obs_dim, units, s.act_dim), sizes=_sizes(RI.mlp_shapes(s.obs_dim, units, s.act_dim)))
        out.append(Check("param", "abs", 0.3 * s.lr, how="ceiling (_check_step)"))
    for c in out:
        if c.key.startswith("param") and c.against == "f64":
            c.against = "f32"
    return out


# ---- derived element-wise bars (the inputs of the stage are exact in these cases) ----------------------------------------------------
def bar_w_clamped(ref):
    """w = clamp(expf(z), 0, max), z exact: expf within 2 ulp of the true value (the f32 result of a correctly implemented expf is good
    to 1 ulp; 4 ulp allowed); below the smallest normal f32 the library may return a subnormal or 0"""
    return 4 * ULP, TINY


def bar_w_clamped_z_rounded(ref):
    """the same where adv = q - v and z = inv_lambda adv are rounded to f32 first (2^-24 |z| each, which expf turns into a relative error)"""
    return 4 * ULP + 2.0 ** -23 * np.abs(10.0 * ref["adv"]), TINY


def bar_w_softmax(ref):
    """w = expf(z - max) / sum: z - max exact, expf 2 ulp, the sum of n positive terms n 2^-24 relative, one division"""
    return 4 * ULP + ref["w"].size * 2.0 ** -24, TINY


def _logp_parts(s, mean, head2, act):
    """float64 pieces of GaussianActor::logp per (row, action column): |c - log std|, q = d^2 / (2 var), |d| (|x| + |mean|) / var, |log(1 - a^2)|"""
    ls = np.clip(np.asarray(head2, np.float64).reshape(1, -1), f32(s.min_log_std), f32(s.max_log_std))
    var = np.exp(2 * ls)
    act, mean = np.asarray(act, np.float64), np.asarray(mean, np.float64)
    if s.action_limit == "Tanh":
        t = np.clip(act / f32(s.action_scale), -CLAMP1, CLAMP1)
        x = 0.5 * np.log((1 + t) / (1 - t))
        lj = np.abs(np.log(1 - np.clip(act, -CLAMP1, CLAMP1) ** 2))
    else:
        x, lj = act, 0 * act
    d = x - mean
    return np.abs(-0.5 * math.log(2 * math.pi) - ls) + 0 * act, 0.5 * d * d / var, np.abs(d) * (np.abs(x) + np.abs(mean)) / var, lj


def logp_magnitude(s, mean, head2, act) -> np.ndarray:
    """per row: the size of the terms that logp adds up, with the conditioning of d = x - mean; a first-order bound on the f32 error of
    logp is a few ulp of this"""
    return sum(_logp_parts(s, mean, head2, act)).sum(-1)


def logp_addend_max(s, mean, head2, act) -> np.ndarray:
    """per row: the largest of the addends that logp sums in f32 (c - log std_j, q_j, log(1 - a_j^2) over the action columns)"""
    c, q, _, lj = _logp_parts(s, mean, head2, act)
    return np.maximum(np.maximum(c, q), lj).max(-1)


def bar_logp(case_spec, mean, head2, act):
    """logp from exact means, exact actions and head2: every primitive (expf, logf, /, *, +) within 2 ulp, 8 ulp of the terms' size"""
    mag = logp_magnitude(case_spec, mean, head2, act)
    return lambda ref: (0.0, 8 * ULP * mag)


# ======================================================================================================== IQL cases
# obs columns: 0 V | 1, 2 target critics | 3, 4 online critics | 5..9 the actor's mean | 10, 11 free (N(0,1), read by the random units)
IQL_O, IQL_A = 12, 5
U_GRID = np.array([-20, -12, -10, -2, -0.5, -1 / 64, 0, 1 / 64, 0.25, 0.5, 2, 9, 10, 12, 20])   # u = adv; inv_lambda 10: z from -200 to 200
D_GRID = np.array([-50, -1.5, -1, -0.5, 0, 0.5, 1, 1.5, 50])                                     # Q - tgt across the SmoothL1 kink
T_GRID = np.array([0, f32(0.9), -f32(0.9), CLAMP1, -CLAMP1, 1, -1, 1.25, -1.25])                 # a / action_scale
C_GRID = np.array([-1, -0.25, 0, 0.25, 0.5, 1])                                                   # Clamp limit: inside, at and outside [-0.25, 0.5]
HEAD2 = np.array([-6.0, -5.0, 0.125, 2.0, 3.0], np.float32)                                      # below, at, inside, at, above [-5, 2]
FLAGS = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.int8)                                       # (is_terminated, is_truncated)


def head2_sides(spec, head2) -> dict:
    """the action columns on each side of the log-std clamp, from the actor's parameters and the spec"""
    h, lo, hi, A = np.asarray(head2, np.float64), f32(spec.min_log_std), f32(spec.max_log_std), len(head2)
    return {"head2 below min": ((h < lo).sum(), A, False), "head2 at min": ((h == lo).sum(), A, False), "head2 inside": (((h > lo) & (h < hi)).sum(), A, False),
            "head2 at max": ((h == hi).sum(), A, False), "head2 above max": ((h > hi).sum(), A, False)}


def _q64(rng, n, lo, hi):
    """multiples of 1/64 in [lo, hi]: few mantissa bits, so sums and differences of them are exact in f32"""
    return rng.integers(int(lo * 64), int(hi * 64) + 1, n) / 64.0


def iql_case(name, branch, muts, *, n=250, tau_iql=0.7, exp_adv_max=100.0, softmax=False, limit="Tanh", scale=2.0, loss="SmoothL1",
             frozen=True, flags="mixed", u=None, mode="dial", relu_out=False, seed=0, steps=1):
    rng = np.random.default_rng(seed)
    O, A = IQL_O, IQL_A
    lr = 0.0 if frozen else 3e-4
    spec = RI.IqlSpec(O, A, (32,), (32, 48), (48, 32), n_critics=2, tau_iql=tau_iql, exp_adv_max=exp_adv_max, adv_softmax=softmax,
                      critic_loss=loss, min_log_std=-5.0, max_log_std=2.0, action_limit=limit, action_min=-0.25, action_max=0.5,
                      action_scale=scale, gamma=0.5, lr_value=lr, lr_critic=lr, critic_tau=0.0 if frozen else 0.005, v_relu_out=relu_out,
                      q_relu_out=relu_out)
    if mode == "zero":   # all weights 0: the losses come from the biases alone
        actor = np.concatenate([const_mlp(O, spec.p_units, A, 0.5, [0.25, -0.5, 0, 1, -1]), np.zeros(A, np.float32)])
        crit = [const_mlp(O + A, spec.q_units, 1, 0.5, [0.75]), const_mlp(O + A, spec.q_units, 1, 0.5, [-1.5])]
        tgts = [const_mlp(O + A, spec.q_units, 1, 0.5, [0.25]), const_mlp(O + A, spec.q_units, 1, 0.5, [0.5])]
        value = const_mlp(O, spec.v_units, 1, 0.5, [0.125])
    else:
        actor = np.concatenate([dial_mlp(O, spec.p_units, A, list(range(5, 10)), rng=rng), HEAD2])
        crit = [dial_mlp(O + A, spec.q_units, 1, [3 + i], rng=rng) for i in range(2)]
        tgts = [dial_mlp(O + A, spec.q_units, 1, [1 + i]) for i in range(2)]
        value = dial_mlp(O, spec.v_units, 1, [0], rng=rng)
    batches = []
    for step in range(steps):
        b = np.arange(n)
        uu = U_GRID[b % len(U_GRID)] if u is None else np.broadcast_to(np.asarray(u, np.float64), (n,)).copy()
        if softmax and u is None:
            uu[:2] = 24.0            # two rows share the whole mass
        v = _q64(rng, n, -2, 2)
        if relu_out:
            v = np.abs(v) * np.where(b % 3 == 0, -1, 1)    # a third of the rows below the output ReLU
        if mode == "relu0":
            v[:] = 0.0               # the value dial's two units sit at pre-activation 0 on every row
        qmin = (np.maximum(v, 0) if relu_out else v) + uu
        q0 = np.where(b % 2 == 0, qmin, qmin + 0.5)
        q1 = np.where(b % 2 == 0, qmin + 1.0, qmin)
        fl = FLAGS[b % 4] if flags == "mixed" else np.ones((n, 2), np.int8)
        vn = _q64(rng, n, -2, 2)
        rew = _q64(rng, n, -1, 1)
        gnd = (1 - (fl[:, 0] | fl[:, 1])) * 0.5
        tgt = rew + gnd * (np.maximum(vn, 0) if relu_out else vn)
        d = D_GRID[b % len(D_GRID)]
        p0, p1 = tgt + d, tgt - d
        if mode == "relu0":
            p0[:] = 0.0
        mean = _q64(rng, (n, A), -1, 1)
        if mode == "relu0":
            mean[:, 0] = 0.0
        if limit == "Tanh":
            act = f32(scale) * T_GRID[(b[:, None] + 2 * np.arange(A)[None, :]) % len(T_GRID)]
        else:
            act = C_GRID[(b[:, None] + np.arange(A)[None, :]) % len(C_GRID)]
        obs = np.concatenate([np.stack([v, q0, q1, p0, p1], 1), mean, rng.standard_normal((n, 2))], 1).astype(np.float32)
        nxt = rng.standard_normal((n, O)).astype(np.float32)
        nxt[:, 0] = vn
        if mode == "zero":
            obs = rng.standard_normal((n, O)).astype(np.float32)
        batches.append((obs, act.astype(np.float32), nxt, rew.astype(np.float32), fl[:, 0].copy(), fl[:, 1].copy()))
    dial = mode != "zero"
    exact = ("q_tgt_min_value", "v", "u", "q_pred") + (("tgt", "v_next", "q_tgt_min_actor", "v_obs") if frozen else ())
    if steps > 1 and not frozen:
        exact = ()
    derived = {}
    if frozen and dial:
        derived["w"] = bar_w_softmax if softmax else bar_w_clamped
        derived["logp"] = bar_logp(spec, batches[-1][0][:, 5:10].astype(np.float64), HEAD2, batches[-1][1])
    zero = {}
    if dial:
        zero["grad_actor"] = len(actor) - A + np.array([0, 4])      # head2 outside [min_log_std, max_log_std]
    hi_z = 88.7 / 10.0
    lnmax = math.log(exp_adv_max) / 10.0

    def coverage(r):
        tot, cov = n, {}
        uu = r["u"]
        if mode == "zero":
            return {"u > 0 (the biases' difference)": ((uu == 0.125).sum(), tot, False)}
        if relu_out:
            return {"V below its output ReLU": ((r["v"] == 0).sum(), tot, False), "V above": ((r["v"] > 0).sum(), tot, False),
                    "Q below its output ReLU": ((r["q_pred"] == 0).sum(), 2 * tot, False), "Q above": ((r["q_pred"] > 0).sum(), 2 * tot, False)}
        if u is None:
            cov.update({"u < 0": ((uu < 0).sum(), tot, False), "u > 0": ((uu > 0).sum(), tot, False), "u == 0": ((uu == 0).sum(), tot, True)})
        adv = r["q_tgt_min_actor"] - r["v_obs"]
        if softmax and u is None:
            cov.update({"exp(z) overflows f32": ((adv > hi_z).sum(), tot, False), "w underflows to 0": ((r["w"] < 2.0 ** -149).sum(), tot, False),
                        "rows that hold the mass": ((r["w"] > 0.4).sum(), tot, True)})
        elif softmax:
            cov["w == 1/B"] = ((np.abs(r["w"] * n - 1) < 1e-12).sum(), tot, False)
        elif u is None:
            cov.update({"w == exp_adv_max": ((r["w"] == f32(exp_adv_max)).sum(), tot, False), "w < exp_adv_max": ((adv < lnmax).sum(), tot, False),
                        "exp(z) overflows f32": ((adv > hi_z).sum(), tot, False), "exp(z) is 0 or subnormal in f32": ((adv * 10 < -87.4).sum(), tot, True)})
        if dial and mode != "relu0":
            dd = r["q_pred"][0] - r["tgt"]
            if loss == "SmoothL1":
                cov.update({"|d| < 1": ((np.abs(dd) < 1).sum(), tot, False), "|d| > 1": ((np.abs(dd) > 1).sum(), tot, False),
                            "|d| == 1": ((np.abs(dd) == 1).sum(), tot, True), "d == 0": ((dd == 0).sum(), tot, True)})
            if limit == "Tanh":
                t = np.abs(batches[-1][1].astype(np.float64) / f32(scale))
                cov.update({"|a/scale| inside the clamp": ((t < CLAMP1).sum(), t.size, False), "|a/scale| at the clamp": ((t == CLAMP1).sum(), t.size, False),
                            "|a/scale| beyond the clamp": ((t > CLAMP1).sum(), t.size, False)})
            else:
                a = batches[-1][1]
                cov.update({"a outside [min, max]": (((a < -0.25) | (a > 0.5)).sum(), a.size, False), "a inside": (((a > -0.25) & (a < 0.5)).sum(), a.size, False)})
            cov.update(head2_sides(spec, actor[-A:]))
        if flags == "mixed":
            f = batches[-1]
            cov.update({"truncated only": (((f[4] == 0) & (f[5] == 1)).sum(), tot, False), "not done": (((f[4] | f[5]) == 0).sum(), tot, False)})
        if not frozen:   # the optimizers move the dials by about lr: the sides placed exactly on a boundary are left to the frozen cases
            cov = {k: v for k, v in cov.items() if not v[2]}
        return cov
    return Case(name, "iql", spec, (actor, crit, tgts, value), batches, branch, coverage, tuple(muts), exact, derived, zero,
                random_units="actor, online critics and value (free hidden units); the target critics are pure dials" if dial else "none")


def iql_cases():
    elem = ("lstd_clamp_dropped", "lstd_grad_open", "lstd_grad_half_open", "lstd_grad_open_interval")
    tanh = ("atanh_clamp_dropped", "jac_clamp_dropped", "jac_on_scaled")
    val = ("expectile_flipped", "expectile_dropped")
    return [
        iql_case("tau07_max100_tanh2", "expectile sides; w clamp at 100 with exp over- and underflow; log-std clamp and mask; atanh / Jacobian clamp, scale 2; SmoothL1 kink; done flags",
                 val + ("w_clamp_dropped",) + elem + tanh + ("huber_quadratic", "huber_linear", "trunc_ignored", "relu0")),
        iql_case("tau05_max1_tanh1", "tau 0.5; w clamp at 1; Tanh limit at scale 1 (a == a / scale)", ("w_clamp_dropped",) + elem + tanh[:2],
                 tau_iql=0.5, exp_adv_max=1.0, scale=1.0, seed=1),
        iql_case("tau099_clamp_mse", "tau 0.99; Clamp limit with actions outside [min, max] (logp takes them as they are); MSE critics",
                 val + ("w_clamp_dropped", "logp_clamps_act") + elem, tau_iql=0.99, limit="Clamp", loss="Mse", seed=2),
        iql_case("softmax_spread", "batch softmax with inv_lambda adv from -200 to 240: two rows hold the mass", ("softmax_no_max",) + elem[:2], softmax=True, seed=3),
        iql_case("softmax_uniform", "batch softmax of equal advantages: 1/B in every row", ("softmax_no_max",), softmax=True, u=12.0, seed=4),
        iql_case("all_done", "is_terminated and is_truncated set in every row: tgt = r", ("done_ignored",), flags="all", seed=5),
        iql_case("relu_out", "output ReLU of V and Q: rows below it get no gradient", ("relu0",), relu_out=True, loss="Mse", seed=6, u=None),
        iql_case("live_two_steps", "the same branches with every optimizer running (lr 3e-4), second step", val + ("w_clamp_dropped",) + elem[:3] + tanh[:2],   # jac_on_scaled: told apart in tau07_max100_tanh2, where logp has its derived bar
                 frozen=False, steps=2, seed=7),
        iql_case("zero_networks", "all weights 0: the losses come from the biases, every hidden gradient is exactly 0", ("expectile_flipped",), mode="zero",
                 frozen=False, seed=8, u=None),
        iql_case("relu_at_zero", "hidden pre-activations exactly 0: V's and critic 0's dial units in every row, the actor's mean-0 dial", ("relu0",), mode="relu0", seed=9),
    ]


# ======================================================================================================== AWAC cases
# obs columns: 0..4 the actor's mean | 5..7 free.  Critic i reads action column i: Q_i(obs, a) = gain a_i, so that Q(obs, act_) follows the
# sampled action; the targets have half the gain.
AWAC_O, AWAC_A = 8, 5


def awac_case(name, branch, muts, *, n=250, exp_adv_max=100.0, softmax=False, limit="Clamp", scale=2.0, loss="SmoothL1", frozen=True,
              flags="mixed", noise=None, mode="dial", gain=64.0, relu_out=False, seed=0, steps=1, uniform=False):
    """noise: None eval mode | "saturate" draws that put every act_ / next_act on the limit | "normal" N(0,1) draws rounded to 1/64"""
    rng = np.random.default_rng(seed)
    O, A = AWAC_O, AWAC_A
    spec = RA.AwacSpec(O, A, (32, 48), (48, 32), n_critics=2, exp_adv_max=exp_adv_max, adv_softmax=softmax, critic_loss=loss, min_log_std=-5.0,
                       max_log_std=2.0, action_limit=limit, action_min=-0.25, action_max=0.5, action_scale=scale, gamma=0.5,
                       lr_actor=0.0 if frozen else 3e-4, q_relu_out=relu_out)
    if mode == "zero":
        actor = np.concatenate([const_mlp(O, spec.p_units, A, 0.5, [0.25, -0.5, 0, 1, -1]), np.zeros(A, np.float32)])
        crit = [const_mlp(O + A, spec.q_units, 1, 0.5, [0.75]), const_mlp(O + A, spec.q_units, 1, 0.5, [-1.5])]
        tgts = [const_mlp(O + A, spec.q_units, 1, 0.5, [0.25]), const_mlp(O + A, spec.q_units, 1, 0.5, [0.5])]
    else:
        actor = np.concatenate([dial_mlp(O, spec.p_units, A, list(range(5)), rng=rng), HEAD2])
        crit = [dial_mlp(O + A, spec.q_units, 1, [O + i], gain=gain, rng=rng) for i in range(2)]
        tgts = [dial_mlp(O + A, spec.q_units, 1, [O + i], gain=gain / 2) for i in range(2)]
    std = np.exp(np.clip(HEAD2.astype(np.float64), -5, 2))
    zsat = np.array([4096.0, 4096.0, 32.0, 4.0, 4.0])     # std z of 27 and more: tanh is +-1 and every clamp is reached, in f32 and in float64
    lim = (lambda a: np.clip(a, -0.25, 0.5)) if limit == "Clamp" else (lambda a: f32(scale) * np.tanh(a))
    batches = []
    for step in range(steps):
        b = np.arange(n)
        mean = _q64(rng, (n, A), -1, 1)
        nmean = _q64(rng, (n, A), -1, 1)
        if mode == "relu0":
            mean[:, 0] = 0.0
        if uniform:
            mean[:, :2] = 0.25
        if noise == "saturate":
            z_pi = zsat * np.where((b[:, None] >> np.arange(A)) & 1 == 0, 1.0, -1.0)
            z_next = zsat * np.where((b[:, None] // 2 + np.arange(A)) % 2 == 0, 1.0, -1.0)
        elif noise == "normal":
            z_pi, z_next = np.round(rng.standard_normal((n, A)) * 64) / 64, np.round(rng.standard_normal((n, A)) * 64) / 64
        else:
            z_pi = z_next = None
        if limit == "Tanh":
            act = f32(scale) * T_GRID[(b[:, None] + 2 * np.arange(A)[None, :]) % len(T_GRID)]
        else:
            act = C_GRID[(b[:, None] + np.arange(A)[None, :] * (1 + b[:, None] // 6)) % len(C_GRID)]
        if uniform:
            act[:, :2] = 0.5
        na = lim(nmean if z_next is None else nmean + std * z_next)
        fl = FLAGS[b % 4] if flags == "mixed" else np.ones((n, 2), np.int8)
        gnd = (1 - (fl[:, 0] | fl[:, 1])) * 0.5
        nq = gain / 2 * np.minimum(na[:, 0], na[:, 1])
        d = D_GRID[b % len(D_GRID)]
        rew = gain * act[:, 0] - d - gnd * nq             # Q_0 - tgt = d where next_act is exact
        if mode == "zero":
            rew = _q64(rng, n, -1, 1)
        obs = np.concatenate([mean, rng.standard_normal((n, 3))], 1).astype(np.float32)
        nxt = np.concatenate([nmean, rng.standard_normal((n, 3))], 1).astype(np.float32)
        f = lambda x: None if x is None else x.astype(np.float32)
        batches.append((obs, act.astype(np.float32), nxt, rew.astype(np.float32), fl[:, 0].copy(), fl[:, 1].copy(), f(z_pi), f(z_next)))
    dial = mode != "zero"
    sampled_exact = limit == "Clamp" and noise is None or noise == "saturate"     # act_ is a dialled mean clamped, or sits on the limit
    exact = ("q_data_min", "q_pred") if dial else ()
    if dial and sampled_exact:   # adv = q - v needs 25 bits where q = gain scale 0.999999 and v = -gain scale: exact under the Clamp limit only
        exact += ("act_", "q_pi_min") + (("adv",) if limit == "Clamp" else ()) + (("next_act", "next_q", "tgt") if frozen or noise == "saturate" else ())
    if steps > 1:
        exact = ()
    derived = {}
    if dial and sampled_exact and steps == 1:
        derived["w"] = bar_w_softmax if softmax else (bar_w_clamped if limit == "Clamp" else bar_w_clamped_z_rounded)
    if dial:
        derived["logp"] = bar_logp(spec, batches[-1][0][:, :5].astype(np.float64), HEAD2, batches[-1][1])
    zero = {"grad_actor": len(actor) - A + np.array([0, 4])} if dial else {}
    il = 10.0

    def coverage(r):
        tot, cov = n, {}
        if mode == "zero":
            return {"adv == 0 (Q does not see the action)": ((r["adv"] == 0).sum(), tot, False)}
        adv = r["adv"]
        if relu_out:
            return {"Q below its output ReLU": ((r["q_pred"] == 0).sum(), 2 * tot, False), "Q above": ((r["q_pred"] > 0).sum(), 2 * tot, False)}
        if uniform:
            return {"w == 1/B": ((np.abs(r["w"] * n - 1) < 1e-12).sum(), tot, False)}
        if softmax:
            cov.update({"exp(z) overflows f32": ((adv * il > 88.7).sum(), tot, False), "w underflows to 0": ((r["w"] < 2.0 ** -149).sum(), tot, False),
                        "rows that hold the mass": ((r["w"] > 0.5 * r["w"].max()).sum(), tot, True)})
        else:
            cov.update({"w == exp_adv_max": ((r["w"] == f32(exp_adv_max)).sum(), tot, False), "w < exp_adv_max": ((r["w"] < f32(exp_adv_max)).sum(), tot, False),
                        "exp(z) is 0 or subnormal in f32": ((adv * il < -87.4).sum(), tot, True)})
            if exp_adv_max > 1:
                cov["exp(z) overflows f32"] = ((adv * il > 88.7).sum(), tot, False)
        dd = r["q_pred"][0] - r["tgt"]
        if loss == "SmoothL1":
            cov.update({"|d| < 1": ((np.abs(dd) < 1).sum(), tot, False), "|d| > 1": ((np.abs(dd) > 1).sum(), tot, False)})
            if "tgt" in exact:
                cov.update({"|d| == 1": ((np.abs(dd) == 1).sum(), tot, True), "d == 0": ((dd == 0).sum(), tot, True)})
        a = batches[-1][1].astype(np.float64)
        if limit == "Tanh":
            t = np.abs(a / f32(scale))
            cov.update({"|a/scale| inside the clamp": ((t < CLAMP1).sum(), t.size, False), "|a/scale| at the clamp": ((t == CLAMP1).sum(), t.size, False),
                        "|a/scale| beyond the clamp": ((t > CLAMP1).sum(), t.size, False)})
            sat = np.abs(r["act_"]) == f32(scale)
        else:
            cov.update({"a outside [min, max]": (((a < -0.25) | (a > 0.5)).sum(), a.size, False), "a inside": (((a > -0.25) & (a < 0.5)).sum(), a.size, False)})
            sat = (r["act_"] == -0.25) | (r["act_"] == 0.5)
        if limit == "Clamp" or noise == "saturate":
            cov["act_ on the limit"] = (sat.sum(), sat.size, False)
        if noise != "saturate":
            cov["act_ inside the limit"] = ((~sat).sum(), sat.size, False)
        cov.update(head2_sides(spec, actor[-A:]))
        if flags == "mixed":
            f = batches[-1]
            cov.update({"truncated only": (((f[4] == 0) & (f[5] == 1)).sum(), tot, False), "not done": (((f[4] | f[5]) == 0).sum(), tot, False)})
        return cov
    return Case(name, "awac", spec, (actor, crit, tgts), batches, branch, coverage, tuple(muts), exact, derived, zero,
                build=dict(train=noise is not None),
                random_units="actor and online critics (free hidden units); the target critics are pure dials" if dial else "none")


def awac_cases():
    elem = ("lstd_clamp_dropped", "lstd_grad_open", "lstd_grad_half_open", "lstd_grad_open_interval")
    tanh = ("atanh_clamp_dropped", "jac_clamp_dropped", "jac_on_scaled")
    return [
        awac_case("clamp_eval_max100", "w clamp at 100 with exp over- and underflow; Clamp limit: act_ = clamp(mean), logp of actions outside [min, max]; log-std clamp and mask; SmoothL1 kink; done flags",
                  ("w_clamp_dropped", "logp_clamps_act", "sample_clamp_dropped", "v_from_targets") + elem + ("huber_quadratic", "huber_linear", "trunc_ignored", "relu0")),
        awac_case("tanh_train_saturated_max1", "train mode, draws that saturate act_ and next_act at +-scale; w clamp at 1; atanh / Jacobian clamp, scale 2",
                  ("w_clamp_dropped",) + elem + tanh + ("huber_quadratic", "trunc_ignored"), limit="Tanh", exp_adv_max=1.0, noise="saturate", gain=8.0, frozen=False, seed=1),
        awac_case("tanh1_eval_mse", "Tanh limit at scale 1, eval mode, MSE critics (summed over the critics)", ("w_clamp_dropped",) + elem[:2] + tanh[:2],
                  limit="Tanh", scale=1.0, loss="Mse", seed=2),
        awac_case("clamp_train_normal", "train mode with N(0,1) draws: std = exp(clamp(head2)) in Policy::sample, the Clamp limit on both sides",
                  ("sample_lstd_clamp_dropped", "sample_clamp_dropped", "w_clamp_dropped"), noise="normal", frozen=False, seed=3),
        awac_case("softmax_spread", "batch softmax with inv_lambda adv spread over more than 200", ("softmax_no_max",) + elem[:2], softmax=True, seed=4),
        awac_case("softmax_uniform", "batch softmax of equal advantages: 1/B in every row", ("softmax_no_max",), softmax=True, uniform=True, seed=5),
        awac_case("all_done", "is_terminated and is_truncated set in every row: tgt = r", ("done_ignored",), flags="all", seed=6),
        awac_case("relu_out", "output ReLU of Q: rows below it get no gradient", ("relu0",), relu_out=True, loss="Mse", seed=7),
        awac_case("live_two_steps", "the same branches with both optimizers running (lr 3e-4), second step", ("w_clamp_dropped",) + elem[:3] + ("huber_linear",),
                  frozen=False, steps=2, seed=8),
        awac_case("zero_networks", "all weights 0: the losses come from the biases, every hidden gradient is exactly 0", ("huber_quadratic",), mode="zero",
                  frozen=False, seed=9),
        awac_case("relu_at_zero", "hidden pre-activations exactly 0: the actor's mean-0 dial in every row", ("relu0",), mode="relu0", seed=10),
    ]


# ======================================================================================================== BC cases
# obs columns: 0..4 dial the five pre-activations | 5..7 free
BC_O, BC_A = 8, 5
Z_GRID = np.array([-100, -20, -1e-3, 0, 1e-3, 20, 100], np.float32).astype(np.float64)
BC_FORMS = ("general", "fused", "fused_mfma")


def bar_bc_pred(ref):
    """tanhf / 1 / (1 + expf(-z)) of an exact z: within 2 ulp each, 4 ulp allowed; sigmoid(-100) = 3.7e-44 is below the smallest normal"""
    return 4 * ULP, TINY


def bar_bc_dz(act_out, act):
    """dz = 2 d inv_n act'(z): d, inv_n and the products round once each (4 ulp relative); for Tanh / Sigmoid act' = 1 - y^2 | y (1 - y)
    carries the absolute error of y near saturation, about 3 ulp of 1, times |2 d inv_n|, and d = y - a carries the error of y (4 ulp of
    |y|) where the two nearly cancel, times 2 inv_n act' <= 2 inv_n"""
    def bar(ref):
        d = ref["pred"] - np.asarray(act, np.float64)
        return 4 * ULP, (4 * ULP * (np.abs(2 * d) + 2 * np.abs(ref["pred"])) / d.size if act_out in ("Tanh", "Sigmoid") else 0.0) + TINY
    return bar


def bc_case(name, branch, muts, act_out, *, n=250, mode="dial", units=(32, 48), seed=0, steps=1, lr=1e-3):
    rng = np.random.default_rng(seed)
    O, A = BC_O, BC_A
    spec = RB.BcSpec(O, A, units, act_out, lr=lr)
    flat = const_mlp(O, units, A, 0.5, [0.25, -0.5, 0, 1, -1]) if mode == "zero" else dial_mlp(O, units, A, list(range(A)), rng=rng)
    batches = []
    for _ in range(steps):
        b = np.arange(n)
        z = Z_GRID[(b[:, None] + 3 * np.arange(A)[None, :]) % len(Z_GRID)]
        if mode == "relu0":
            z[:, 0] = 0.0
        obs = np.concatenate([z, rng.standard_normal((n, 3))], 1).astype(np.float32)
        act = _q64(rng, (n, A), -1, 1).astype(np.float32)
        batches.append((obs, act))
    dial = mode != "zero"
    exact = ("pred",) if dial and steps == 1 and act_out in ("None", "ReLU") else ()
    derived = {}
    if dial and steps == 1:   # after a step the pre-activations are no longer the dialled columns
        if act_out in ("Tanh", "Sigmoid"):
            derived["pred"] = bar_bc_pred
        derived["dz"] = bar_bc_dz(act_out, batches[-1][1])
    zero = {}
    if mode == "relu0":   # the dial units of column 0 sit at pre-activation 0 in every row: their two rows of the first weight gradient
        zero["grad"] = np.arange(2 * O)

    def coverage(r):
        if mode == "zero":
            return {"rows whose pre-activation is the bias alone": ((r["z"] == np.array([0.25, -0.5, 0, 1, -1])).all(1).sum(), n, False)}
        z = r["z"]
        cov = {"z < 0": ((z < 0).sum(), z.size, False), "z > 0": ((z > 0).sum(), z.size, False), "z == 0": ((z == 0).sum(), z.size, True),
               "|z| >= 20": ((np.abs(z) >= 20).sum(), z.size, False), "|z| <= 1e-3": ((np.abs(z) < 0.01).sum(), z.size, False)}
        if mode == "relu0":
            cov["rows with both dial units of column 0 at 0"] = ((z[:, 0] == 0).sum(), n, False)
        if steps > 1:
            cov = {k: v for k, v in cov.items() if not v[2] and k != "|z| <= 1e-3"}
        return cov
    return Case(name, "bc", spec, (flat,), batches, branch, coverage, tuple(muts), exact, derived, zero,
                random_units="the policy's free hidden units" if dial else "none")


def bc_cases():
    return [
        bc_case("none", "no output activation: pred = z, dz = 2 d / n", ("relu0",), "None"),
        bc_case("relu", "output ReLU and its derivative at z = 0 and on both sides", ("relu0", "out_act_dropped"), "ReLU", seed=1),
        bc_case("tanh", "Tanh saturating to +-1 (derivative exactly 0 from |z| = 20) and linear at 1e-3", ("tanh_grad_of_z", "out_act_dropped"), "Tanh", seed=2),
        bc_case("sigmoid", "Sigmoid from exp(100) (overflow in e / (1 + e)) to exp(-100)", ("sigmoid_e_over_1pe", "sigmoid_grad_y", "out_act_dropped"), "Sigmoid", seed=3),
        bc_case("sigmoid_one_hidden_two_steps", "the same on one hidden layer, second step of a running optimizer", ("sigmoid_e_over_1pe",), "Sigmoid", units=(64,), steps=2, seed=4),
        bc_case("zero_networks", "all weights 0: the loss comes from the biases, every hidden gradient is exactly 0", ("out_act_dropped",), "Tanh", mode="zero", seed=5),
        bc_case("relu_at_zero", "hidden pre-activations exactly 0 in both dial units of column 0 on every row: relu'(0) = 0 zeroes two rows of dW0", ("relu0",), "None",
                mode="relu0", seed=6),
    ]



# ======================================================================================================== SAC
@dataclass
class SacSpec:
    obs_dim: int
    act_dim: int
    pi_units: Sequence[int] = (64, 64)
    q_units: Sequence[int] = (64, 64)
    n_critics: int = 2
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    gamma: float = 0.99
    tau: float = 0.005
    ent_coef: tuple = ("Fix", 1.0)
    epsilon: float = 1e-4
    min_lstd: float = -20.0
    max_lstd: float = 2.0
    reward_scale: float = 1.0
    critic_loss: str = "Mse"

    def to_config(self, B, batch_size: int, **kw):
        return B.SacConfig(obs_dim=self.obs_dim, act_dim=self.act_dim, pi_units=tuple(self.pi_units), q_units=tuple(self.q_units),
                           lr_actor=self.lr_actor, lr_critic=self.lr_critic, gamma=self.gamma, tau=self.tau, ent_coef_mode=self.ent_coef,
                           epsilon=self.epsilon, min_lstd=self.min_lstd, max_lstd=self.max_lstd, critic_loss=self.critic_loss,
                           reward_scale=self.reward_scale, n_critics=self.n_critics, batch_size=batch_size, **kw)


def _unflat(flat, shapes, dtype, grad=True):
    ts, o = [], 0
    for sh in shapes:
        n = int(np.prod(sh))
        ts.append(torch.tensor(np.asarray(flat[o:o + n], np.float32).reshape(sh), dtype=dtype, requires_grad=grad))
        o += n
    assert o == len(flat), (o, len(flat))
    return ts


def _flat64(ts, grad=False):
    return np.concatenate([(t.grad if grad else t).detach().numpy().reshape(-1) for t in ts]).astype(np.float64)


def _mlp(p, x, mut=(), relu_out=False):
    relu = relu_grad1_at_0 if "relu0" in mut else torch.relu
    n = len(p) // 2
    for k in range(n):
        x = x @ p[2 * k].T + p[2 * k + 1]
        if k < n - 1 or relu_out:
            x = relu(x)
    return x


class SacRef:
    """Sac::opt_ (sac/base.rs:73-198) in float64, the reference's definitions kept: lstd = exp(head2) is exponentiated again after its
    clip (mlp2.rs:23-28, base.rs:78), log p takes ln(1 - a^2 + eps), EntCoef::update runs before alpha is used"""

    def __init__(self, spec: SacSpec, pi, qs, qs_tgt, mut=(), dtype=DT):
        s = self.spec = spec
        self.T, self.mut, self.dtype = T, frozenset(mut), dtype
        self.n_trunk = len(s.pi_units)
        self.pi = _unflat(pi, T.sac_pi_shapes(s.obs_dim, s.pi_units, s.act_dim), dtype)
        qsh = T.sac_q_shapes(s.obs_dim, s.act_dim, s.q_units)
        self.qs = [_unflat(q, qsh, dtype) for q in qs]
        self.qs_tgt = [_unflat(q, qsh, dtype, grad=False) for q in qs_tgt]
        auto = s.ent_coef[0] == "Auto"
        self.log_alpha = torch.zeros(1, dtype=dtype, requires_grad=True) if auto else torch.tensor([f32(math.log(s.ent_coef[1]))], dtype=dtype)
        st = lambda ps, lr: dict(m=[torch.zeros_like(p) for p in ps], v=[torch.zeros_like(p) for p in ps], vmax=[torch.zeros_like(p) for p in ps], step=0, lr=lr)
        self.opt = {"pi": st(self.pi, s.lr_actor), "alpha": st([self.log_alpha], s.ent_coef[2] if auto else 0.0)}
        for i, q in enumerate(self.qs):
            self.opt[f"q{i}"] = st(q, s.lr_critic)

    def _adam(self, params, st):
        st["step"] += 1
        self.T.optimizer_step(params, st["m"], st["v"], st["vmax"], st["step"], st["lr"], None)

    def action_logp(self, o, z):
        s, mut = self.spec, self.mut
        relu = relu_grad1_at_0 if "relu0" in mut else torch.relu
        x = o
        for i in range(self.n_trunk):
            x = relu(x @ self.pi[2 * i].T + self.pi[2 * i + 1])
        k = 2 * self.n_trunk
        mean, head2 = x @ self.pi[k].T + self.pi[k + 1], x @ self.pi[k + 2].T + self.pi[k + 3]
        lo, hi = f32(s.min_lstd), f32(s.max_lstd)
        lstd = head2 if "single_exp" in mut else head2.exp()
        c = lstd.clamp(lo, hi)
        if "lstd_clip_dropped" in mut:
            c = lstd
        elif "lstd_clip_grad_open" in mut:
            c = lstd + (c - lstd).detach()
        elif "lstd_clip_grad_half_open" in mut:
            c = c.detach() + (lstd - lstd.detach()) * ((lstd >= lo) & (lstd < hi)).to(lstd.dtype)
        std = c.exp()
        pre = std * z + mean
        a = pre.tanh()
        eps = 0.0 if "eps_dropped" in mut else f32(1e-4) if "eps_default" in mut else f32(s.epsilon)
        nl = (f32(-0.5 * math.log(2.0 * math.pi)) - 0.5 * z ** 2).sum(-1)
        log_p = nl - (1.0 - a ** 2 + eps).log().sum(-1)
        return a, log_p, pre

    def q_forward(self, q, o, a):
        return _mlp(q, torch.cat([o, a], -1), self.mut).squeeze(-1)

    def update(self, obs, act, next_obs, reward, term, z_actor, z_next, terms=False) -> dict:
        s, mut = self.spec, self.mut
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32), dtype=self.dtype)
        o, act, no, reward, z_actor, z_next = t(obs), t(act), t(next_obs), t(reward), t(z_actor), t(z_next)
        n = o.shape[0]
        not_term = torch.as_tensor(1.0 - (0 * np.asarray(term) if "term_ignored" in mut else np.asarray(term)).astype(np.float64), dtype=self.dtype)
        out, tm = {}, {}
        a, log_p, pre = self.action_logp(o, z_actor)
        alpha_old = self.log_alpha.detach().exp()
        if s.ent_coef[0] == "Auto":
            loss_a = -(self.log_alpha * (log_p.detach() + f32(s.ent_coef[1]))).mean()
            self.log_alpha.grad = None
            loss_a.backward()
            self._adam([self.log_alpha], self.opt["alpha"])
        alpha = alpha_old if "alpha_before_update" in mut else self.log_alpha.detach().exp()
        q_pi = torch.stack([self.q_forward(q, o, a) for q in self.qs])
        la = (alpha * log_p - q_pi.min(0)[0]) / n
        if terms:
            tm["grad_pi"] = row_terms(la, self.pi)
        for p in self.pi:
            p.grad = None
        la.sum().backward()
        out.update(log_p=log_p, q_pi=q_pi, pre=pre, a=a, loss_actor=la.sum(), terms_loss_actor=la, grad_pi=_flat64(self.pi, True), ent_coef=alpha[0])
        self._adam(self.pi, self.opt["pi"])
        preds = [self.q_forward(q, o, act) for q in self.qs]
        with torch.no_grad():
            next_a, next_log_p, next_pre = self.action_logp(no, z_next)
            q_next = torch.stack([self.q_forward(q, no, next_a) for q in self.qs_tgt])
            qmin = q_next.min(0)[0]
            tgt = f32(s.reward_scale) * reward + not_term * f32(s.gamma) * (qmin - alpha * next_log_p)
        nc = len(preds)
        rows = [(((p - tgt) ** 2) if s.critic_loss == "Mse" else smooth_l1_rows(p, tgt, mut)) / n for p in preds]
        for i, q in enumerate(self.qs):
            if terms:
                tm[f"grad_q_{i}"] = row_terms(rows[i], q)
            for p in q:
                p.grad = None
            rows[i].sum().backward()
            out[f"grad_q_{i}"] = _flat64(q, True)
            self._adam(q, self.opt[f"q{i}"])
        with torch.no_grad():
            for qt, q in zip(self.qs_tgt, self.qs):
                for d, src in zip(qt, q):
                    d.copy_(f32(s.tau) * src + (1.0 - f32(s.tau)) * d)
        lq = torch.stack(rows) / nc
        out.update(q_pred=torch.stack(preds), next_act=next_a, next_log_p=next_log_p, next_pre=next_pre, q_next=q_next, qvals_min=qmin, tgt=tgt,
                   loss_critic=lq.sum(), terms_loss_critic=lq.reshape(-1), param_pi=_flat64(self.pi), log_alpha=self.log_alpha.detach()[0])
        for i in range(nc):
            out[f"param_q_{i}"], out[f"param_q_tgt_{i}"] = _flat64(self.qs[i]), _flat64(self.qs_tgt[i])
        out = {k: (v.detach().numpy().astype(np.float64) if torch.is_tensor(v) else v) for k, v in out.items()}
        out["row_terms"] = tm
        return out


def sac_f32(spec: SacSpec, params, batches) -> dict:
    """oracle.torch_ref.TorchSac (f32) on the same case, under SacRef's keys; it keeps no probe of q_pi / q_next / next_log_p"""
    pi, qs, qs_tgt = params
    r = T.TorchSac(spec.obs_dim, spec.act_dim, list(spec.pi_units), list(spec.q_units), pi, qs, lr_actor=spec.lr_actor, lr_critic=spec.lr_critic,
                   gamma=spec.gamma, tau=spec.tau, ent_coef=spec.ent_coef, epsilon=spec.epsilon, min_lstd=spec.min_lstd, max_lstd=spec.max_lstd,
                   reward_scale=spec.reward_scale, critic_loss=spec.critic_loss)
    r.qs_tgt = [T.unflatten(q, r.q_shapes) for q in qs_tgt]
    for b in batches:
        o = r.update(*b)
    out = dict(log_p=o["log_p"], tgt=o["tgt"], q_pred=np.stack(o["preds"]), loss_critic=o["loss_critic"], loss_actor=o["loss_actor"],
               ent_coef=o["ent_coef"], grad_pi=o["pi_grads"], param_pi=o["pi_params"], log_alpha=o["log_alpha"])
    for i in range(spec.n_critics):
        out[f"grad_q_{i}"], out[f"param_q_{i}"], out[f"param_q_tgt_{i}"] = o["q_grads"][i], o["q_params"][i], o["q_tgt_params"][i]
    return out


def bar_sac_logp(eps, pre_key, z):
    """log p = sum(c - z^2 / 2) - sum ln(1 - a^2 + eps), a = tanhf(x), x = std z + mean from exact inputs.  Where |x| > 9.02 f32 holds
    a == +-1 exactly and the term is ln(eps); float64 still sees 1 - a^2 > 0 there: (1 - a^2) / (1 - a^2 + eps) is allowed for that.
    Elsewhere tanhf within 2 ulp and x within 2 ulp give (4 a^2 + 4 |a x| (1 - a^2) + 1) ulp / (1 - a^2 + eps); logf and the
    Gaussian term 2 ulp of their size; the whole doubled for the order of the sums."""
    def bar(ref):
        x = ref[pre_key]
        a2 = np.tanh(x) ** 2
        sat = np.abs(x) > 9.02
        gap = (1 - a2) / (1 - a2 + eps)
        cond = (4 * a2 + 4 * np.sqrt(a2) * np.abs(x) * (1 - a2) + 1) / (1 - a2 + eps) + 2 * np.abs(np.log(1 - a2 + eps))
        per = np.where(sat, gap + 2 * ULP * abs(math.log(eps)), ULP * cond) + 2 * ULP * (0.92 + 0.5 * np.asarray(z, np.float64) ** 2)
        return 0.0, 2 * per.sum(-1)
    return bar


# obs columns: 0..3 the mean heads | 4..7 the std heads (head2) | 8, 9 the critics' state term | 10, 11 free.
# Critic i: Q_i(o, a) = o[8 + i] + gain a_i (exact where one of the two terms is 0: the batch actions have columns 0, 1 at 0).
SAC_O, SAC_A = 12, 4
H2_GRID = np.array([-1.0, 0.0, 1.0, -100.0])     # exp(head2) inside (0.37), at (1 = max_lstd), above (2.72) and far below: the clip's lower end
                                                  # (min_lstd < 0 < exp(head2)) cannot be reached


def sac_case(name, branch, muts, *, n=250, epsilon=1e-4, ent=("Fix", 0.25), loss="SmoothL1", mode="dial", seed=0, steps=1, gain=4.0, lr=3e-4,
             pi_units=(64, 48), q_units=(48, 32)):
    rng = np.random.default_rng(seed)
    O, A = SAC_O, SAC_A
    # The dial cases hold the actor still (lr_actor = 0; its gradient is still formed and compared): next_act, next_log_p and the TD target
    # are taken after the actor's Adam step, and on the saturated elements, whose gradient is exactly 0 in f32 and 1e-10 in float64, an
    # f32 and a float64 Adam step differ by up to lr, which is not what these cases are about.  zero_networks runs every optimizer.
    spec = SacSpec(O, A, tuple(pi_units), tuple(q_units), 2, lr_actor=lr if mode == "zero" else 0.0, lr_critic=lr, gamma=0.5, ent_coef=ent, epsilon=epsilon, min_lstd=-20.0, max_lstd=1.0,
                   critic_loss=loss)
    if mode == "zero":
        pi = const_mlp(O, spec.pi_units, 2 * A, 0.5, [0.25, -0.5, 0, 1, -1, 0, 1, -100])
        qs = [const_mlp(O + A, spec.q_units, 1, 0.5, [0.75]), const_mlp(O + A, spec.q_units, 1, 0.5, [-1.5])]
        tg = [const_mlp(O + A, spec.q_units, 1, 0.5, [0.25]), const_mlp(O + A, spec.q_units, 1, 0.5, [0.5])]
    else:
        pi = dial_mlp(O, spec.pi_units, 2 * A, list(range(2 * A)), rng=rng)
        qs = [dial_mlp(O + A, spec.q_units, 1, [[(8 + i, 1.0), (O + i, gain)]], rng=rng) for i in range(2)]
        tg = [dial_mlp(O + A, spec.q_units, 1, [[(8 + i, 1.0), (O + i, gain / 2)]]) for i in range(2)]
    # the flat actor holds the trunk, then ml.weight, ml.bias, sl.weight, sl.bias: split the dial's last layer (rows 0..A-1 | A..2A-1)
    w, b = layer_slices(O, spec.pi_units, 2 * A)[-1]
    K = spec.pi_units[-1]
    W, bb = pi[w].reshape(2 * A, K), pi[b]
    pi = np.concatenate([pi[:w.start], W[:A].reshape(-1), bb[:A], W[A:].reshape(-1), bb[A:]]).astype(np.float32)
    # saturated elements: |std z + mean| >= 11.8 with means of +-12, where a == +-1.0f and float64 has 1 - a^2 = 2e-10 (2e-6 of the default
    # epsilon); with epsilon = 1e-6 the means are +-16 (1 - a^2 = 7e-14), so that float64 is a reference for the f32 definition there too
    sat_mean = 12.0 if epsilon > 1e-5 else 16.0
    batches = []
    for _ in range(steps):
        b_ = np.arange(n)

        def side(shift):
            sat = (b_[:, None] + np.arange(A) + shift) % 3 == 0
            mean = np.where(sat, sat_mean * np.where((b_[:, None] // 3 + np.arange(A)) % 2 == 0, 1, -1), _q64(rng, (n, A), -0.5, 0.5))
            h2 = H2_GRID[(b_[:, None] + 2 * np.arange(A) + shift) % 4]
            z = np.where(sat, _q64(rng, (n, A), -1 / 16, 1 / 16), _q64(rng, (n, A), -0.5, 0.5))
            return mean, h2, z
        m1, h1, z1 = side(0)
        m2, h2, z2 = side(1)
        if mode == "relu0":
            m1[:, 0] = 0.0
        fl = (b_ % 2).astype(np.int8)                       # every other row terminated: tgt = r there, Q - tgt = d exactly
        d = D_GRID[(b_ // 2) % len(D_GRID)]
        qcol = _q64(rng, (n, 2), -2, 2)
        rew = np.where(fl == 1, qcol[:, 0] - d, _q64(rng, n, -1, 1))
        act = _q64(rng, (n, A), -1, 1)
        act[:, :2] = 0.0
        obs = np.concatenate([m1, h1, qcol, rng.standard_normal((n, 2))], 1).astype(np.float32)
        nxt = np.concatenate([m2, h2, _q64(rng, (n, 2), -2, 2), rng.standard_normal((n, 2))], 1).astype(np.float32)
        if mode == "zero":
            obs, nxt = rng.standard_normal((n, O)).astype(np.float32), rng.standard_normal((n, O)).astype(np.float32)
        batches.append((obs, act.astype(np.float32), nxt, rew.astype(np.float32), fl, z1.astype(np.float32), z2.astype(np.float32)))
    dial = mode != "zero" and steps == 1
    exact = ("q_pred",) if dial else ()
    derived = {}
    if dial:
        derived["log_p"] = bar_sac_logp(f32(epsilon), "pre", batches[-1][5])
        derived["next_log_p"] = bar_sac_logp(f32(epsilon), "next_pre", batches[-1][6])

    def coverage(r):
        if mode == "zero":
            return {"rows whose Q is the bias alone": ((r["q_pred"][0] == 0.75).sum(), n, False)}
        x = r["pre"]
        cov = {"a == +-1 (|x| > 9.02)": ((np.abs(x) > 9.02).sum(), x.size, False), "|a| < 0.96": ((np.abs(x) < 2).sum(), x.size, False)}
        if steps == 1:
            e = np.exp(batches[-1][0][:, 4:8].astype(np.float64))
            cov.update({"exp(head2) inside": (((e < 1) & (e > 1e-3)).sum(), e.size, False), "exp(head2) at max_lstd": ((e == 1).sum(), e.size, False),
                        "exp(head2) above max_lstd": ((e > 1).sum(), e.size, False), "head2 = -100": ((e < 1e-30).sum(), e.size, False)})
            dd = (r["q_pred"][0] - r["tgt"])[batches[-1][4] == 1]
            if loss == "SmoothL1":
                cov.update({"|d| < 1": ((np.abs(dd) < 1).sum(), dd.size, False), "|d| > 1": ((np.abs(dd) > 1).sum(), dd.size, False),
                            "|d| == 1": ((np.abs(dd) == 1).sum(), dd.size, True), "d == 0": ((dd == 0).sum(), dd.size, True)})
        cov["terminated"] = ((batches[-1][4] == 1).sum(), n, False)
        cov["not terminated"] = ((batches[-1][4] == 0).sum(), n, False)
        return cov
    return Case(name, "sac", spec, (pi, qs, tg), batches, branch, coverage, tuple(muts), exact, derived, {},
                random_units="actor trunk and online critics (free hidden units); the target critics are pure dials" if mode != "zero" else "none")


def sac_cases():
    clip = ("single_exp", "lstd_clip_dropped", "lstd_clip_grad_open", "lstd_clip_grad_half_open")
    return [
        sac_case("fix_alpha_eps_default", "double exponential and its clip (inside, at, above, head2 = -100); a == +-1 with ln(eps) and no gradient through tanh; SmoothL1 kink; terminated rows",
                 clip + ("eps_dropped", "huber_quadratic", "huber_linear", "term_ignored", "relu0")),
        sac_case("auto_alpha_eps_1e-6", "epsilon 1e-6; EntCoef::update with the saturated rows in the mean, alpha used after its step",
                 clip[:2] + ("eps_default", "eps_dropped", "alpha_before_update"), epsilon=1e-6, ent=("Auto", -4.0, 1e-2), seed=1),
        sac_case("auto_alpha_mse", "MSE critics with the automatic entropy coefficient at the default epsilon", clip[:2] + ("alpha_before_update", "term_ignored"),
                 ent=("Auto", -4.0, 1e-2), loss="Mse", seed=2),
        sac_case("fix_alpha_wide_256", "the first case at the default width: 256-wide first layers, which the two-layer chain kernel takes (dense_chain.hpp)",
                 clip[:2] + ("eps_dropped", "huber_linear"), pi_units=(256, 64), q_units=(256, 64), seed=5),
        sac_case("zero_networks", "all weights 0: the losses come from the biases, every hidden gradient is exactly 0", ("single_exp", "eps_dropped"), mode="zero", seed=3),
        sac_case("relu_at_zero", "hidden pre-activations exactly 0: the dial units of mean column 0 in every row", ("relu0",), mode="relu0", seed=4),
    ]



# ======================================================================================================== DQN
@dataclass
class DqnSpec:
    kind: str                      # "mlp" | "cnn"
    n_actions: int
    in_dim: int = 0
    units: Sequence[int] = ()
    lr: float = 1e-3
    gamma: float = 0.5
    double_dqn: bool = False
    critic_loss: str = "SmoothL1"
    clip_td_err: object = None
    tau: float = 0.01
    arithmetic: str = "bf16x3_6"

    def shapes(self):
        return T.mlp_shapes(self.in_dim, list(self.units), self.n_actions) if self.kind == "mlp" else T.cnn_shapes(self.n_actions)

    def to_config(self, B, batch_size: int, **kw):
        q = B.MlpConfig(in_dim=self.in_dim, units=tuple(self.units), out_dim=self.n_actions) if self.kind == "mlp" else B.AtariCnnConfig(out_dim=self.n_actions)
        return B.DqnConfig(model_config=B.DqnModelConfig(q_config=q, opt_config=B.OptimizerConfig.Adam(self.lr)), batch_size=batch_size,
                           discount_factor=self.gamma, double_dqn=self.double_dqn, critic_loss=self.critic_loss, clip_td_err=self.clip_td_err,
                           tau=self.tau, soft_update_interval=1, arithmetic=self.arithmetic, **kw)


class DqnRef:
    """Dqn::update_critic and opt_ (dqn/base.rs:60-160, 190-196) in float64; weight given = the importance-weighted branch (:123-145)"""

    def __init__(self, spec: DqnSpec, q, q_tgt, mut=(), dtype=DT):
        self.spec, self.mut, self.dtype = spec, frozenset(mut), dtype
        self.q = _unflat(q, spec.shapes(), dtype)
        self.q_tgt = _unflat(q_tgt, spec.shapes(), dtype, grad=False)
        self.st = dict(m=[torch.zeros_like(p) for p in self.q], v=[torch.zeros_like(p) for p in self.q], vmax=[torch.zeros_like(p) for p in self.q], step=0)

    def fwd(self, p, x):
        if self.spec.kind == "mlp":
            return _mlp(p, x, self.mut)
        import torch.nn.functional as F
        relu = relu_grad1_at_0 if "relu0" in self.mut else torch.relu
        x = x.squeeze(2) / 255
        x = relu(F.conv2d(x, p[0], p[1], stride=4))
        x = relu(F.conv2d(x, p[2], p[3], stride=2))
        x = relu(F.conv2d(x, p[4], p[5], stride=1)).flatten(1)
        return relu(x @ p[6].T + p[7]) @ p[8].T + p[9]

    def update(self, obs, act, next_obs, reward, term, weight=None, terms=False) -> dict:
        s, mut = self.spec, self.mut
        t = lambda x: torch.as_tensor(np.asarray(x).astype(np.float64), dtype=self.dtype)
        obs, next_obs, reward = t(obs), t(next_obs), t(np.asarray(reward, np.float32))
        act = torch.as_tensor(np.asarray(act, np.int64)).reshape(-1, 1)
        n = len(reward)
        not_term = t(1 - (0 * np.asarray(term) if "term_ignored" in mut else np.asarray(term)))
        q_all = self.fwd(self.q, obs)
        pred = q_all.gather(-1, act).squeeze(-1)
        pick = (lambda x: x.shape[-1] - 1 - x.flip(-1).argmax(-1)) if "argmax_last" in mut else (lambda x: x.argmax(-1))   # ties: the first index
        with torch.no_grad():
            qn_all = self.fwd(self.q_tgt, next_obs)
            y = pick(self.fwd(self.q, next_obs) if s.double_dqn and "ddqn_dropped" not in mut else qn_all).unsqueeze(-1)
            tgt = reward + not_term * f32(s.gamma) * qn_all.gather(-1, y).squeeze(-1)
        d = pred - tgt
        if weight is not None:
            td = d.abs()
            if "abs_grad1_at_0" in mut:     # sgn(0) = 1
                td = torch.where(d >= 0, d, -d)
            if s.clip_td_err is not None and "clip_dropped" not in mut:
                lo, hi = f32(s.clip_td_err[0]), f32(s.clip_td_err[1])
                c = td.clamp(lo, hi)
                if "clip_grad_open" in mut:
                    c = td + (c - td).detach()
                elif "clip_grad_half_open" in mut:
                    c = c.detach() + (td - td.detach()) * ((td >= lo) & (td < hi)).to(td.dtype)
                elif "clip_grad_open_interval" in mut:
                    c = c.detach() + (td - td.detach()) * ((td > lo) & (td < hi)).to(td.dtype)
                td = c
            w = t(np.asarray(weight, np.float32))
            x = td if "weight_dropped" in mut else w * td
            rows = (smooth_l1_rows(x, torch.zeros_like(x), mut) if s.critic_loss == "SmoothL1" else x ** 2) / n
            td_abs = td.detach()
        else:
            rows = (smooth_l1_rows(pred, tgt, mut) if s.critic_loss == "SmoothL1" else d ** 2) / n
            td_abs = d.detach().abs()
        tm = {}
        if terms:
            tm["grad"], tm["grad_entry_max"] = row_terms(rows, self.q, entries=True)
        for p in self.q:
            p.grad = None
        rows.sum().backward()
        out = dict(loss=rows.sum(), terms_loss=rows, q_pred_all=q_all, q_next_all=qn_all, pred=pred, tgt=tgt, td_errs=td_abs, grad=_flat64(self.q, True))
        self.st["step"] += 1
        T.optimizer_step(self.q, self.st["m"], self.st["v"], self.st["vmax"], self.st["step"], s.lr, None)
        with torch.no_grad():
            for dd, src in zip(self.q_tgt, self.q):
                dd.copy_(f32(s.tau) * src + (1.0 - f32(s.tau)) * dd)
        out.update(param=_flat64(self.q), param_tgt=_flat64(self.q_tgt))
        out = {k: (v.detach().numpy().astype(np.float64) if torch.is_tensor(v) else v) for k, v in out.items()}
        out["row_terms"] = tm
        return out


def dqn_f32(spec: DqnSpec, params, batches) -> dict:
    q, q_tgt = params
    r = T.TorchDqn(spec.kind, spec.shapes(), q, lr=spec.lr, discount_factor=spec.gamma, double_dqn=spec.double_dqn, critic_loss=spec.critic_loss,
                   clip_td_err=spec.clip_td_err, tau=spec.tau, soft_update_interval=1)
    r.q_tgt = T.unflatten(q_tgt, spec.shapes())
    for b in batches:
        o = r.update(*b)
    out = dict(loss=o["loss"], q_pred_all=o["q_pred_all"], q_next_all=o["q_next_all"], pred=o["pred"], tgt=o["tgt"], grad=o["grads"],
               param=r.params(), param_tgt=r.tgt_params())
    if o["td_abs"] is not None:
        out["td_errs"] = o["td_abs"]
    return out


# Mlp: obs columns 0..2 dial Q(obs) of the online net and (on next_obs) its double-DQN choice | 3..5 the target net's Q(next_obs) | 6, 7 free
DQN_A = 3
E1, E2 = 2.0 ** -24, 2.0 ** -23
HUBER_D = np.array([0, 1 - E1, -(1 - E1), 1, -1, 1 + E2, -(1 + E2), 50, -50, 0.5, -0.25])   # |d| in {0, 1 - 2^-24, 1, 1 + 2^-23, 50} and two inside
CNN_D = np.array([0, 0.5, -0.25, 1, -1, 50, -50, 2, -3])
CLIP = (0.25, 4.0)
CLIP_D = np.array([0, 0.125, -0.125, 0.25, -0.25, 1, -1, 4, -4, 8, -8])                       # below, at cmin, inside, at cmax, above
PER_W = np.array([0, 1e-30, 1, 1e3])


def dqn_case(name, branch, muts, *, kind="mlp", n=250, double_dqn=True, loss="SmoothL1", clip=None, weighted=False, dgrid=HUBER_D, all_term=False,
             ties=False, mode="dial", arithmetic="bf16x3_6", units=(64, 64), seed=0, d0_all=False):
    rng = np.random.default_rng(seed)
    A = DQN_A if kind == "mlp" else 6
    spec = DqnSpec(kind, A, in_dim=2 * A + 2, units=units, double_dqn=double_dqn, critic_loss=loss, clip_td_err=clip, arithmetic=arithmetic,
                   lr=1e-3 if kind == "mlp" else 1e-4)
    b = np.arange(n)
    act = b % A
    term = np.ones(n, np.int8) if all_term else (b % 4 == 0).astype(np.int8)
    d = np.zeros(n) if d0_all else dgrid[b % len(dgrid)]
    knife = np.abs(d * 64 - np.round(d * 64)) > 0                     # |d| = 1 - 2^-24, 1 + 2^-23: exact only against tgt = 0
    if kind == "mlp":
        if mode == "zero":
            q, qt = const_mlp(spec.in_dim, units, A, 0.5, [0.25, -0.5, 1.0]), const_mlp(spec.in_dim, units, A, 0.5, [0.5, 0.75, -1.0])
        else:
            q = dial_mlp(spec.in_dim, units, A, list(range(A)), rng=rng)
            qt = dial_mlp(spec.in_dim, units, A, list(range(A, 2 * A)))
        qn_on = _q64(rng, (n, A), -2, 2)
        qn_tg = _q64(rng, (n, A), -2, 2)
        if ties:   # the online net's two largest next-state values are equal in every row: the reference takes the first
            qn_on = np.tile(np.array([[1.0, 1.0, 0.5]]), (n, 1))
            qn_on[b % 2 == 1] = np.array([0.25, 1.5, 1.5])
        sel = (qn_on if double_dqn else qn_tg).argmax(1)
        qsel = qn_tg[b, sel]
        rew = _q64(rng, n, -1, 1)
        rew[knife], qn_tg[knife, sel[knife]] = 0.0, 0.0
        if not double_dqn:   # keep the selected entry the maximum
            qn_tg[knife] = np.minimum(qn_tg[knife], 0.0)
            qn_tg[knife, sel[knife]] = 0.0
        tgt = rew + (1 - term) * 0.5 * qn_tg[b, sel]
        qo = _q64(rng, (n, A), -2, 2)
        qo[b, act] = tgt + d
        if mode == "relu0":
            qo[:, 0] = 0.0
        obs = np.concatenate([qo, rng.standard_normal((n, A + 2))], 1).astype(np.float32)
        nxt = np.concatenate([qn_on, qn_tg, rng.standard_normal((n, 2))], 1).astype(np.float32)
        if mode == "zero":
            obs, nxt = rng.standard_normal((n, spec.in_dim)).astype(np.float32), rng.standard_normal((n, spec.in_dim)).astype(np.float32)
    else:   # Nature-CNN: the trunk stays random, the head is dialled: l2.weight = 0, Q = l2.bias in every row, d set through the reward
        sh = T.cnn_shapes(A)
        q = T.init_params(sh, 5 + seed)
        nb = A * 512 + A
        bias_q = np.array([0.5, -1.0, 2.0, 0.0, 1.0, -0.25])
        bias_t = np.array([1.0, 1.0, 0.5, -2.0, 0.0, 0.25]) if ties else np.array([0.25, 1.5, 0.5, -2.0, 0.0, 1.0])
        q[-nb:] = np.concatenate([np.zeros(A * 512), bias_q]).astype(np.float32)
        qt = q.copy()
        qt[-A:] = bias_t
        sel = int(np.argmax(bias_q)) if double_dqn else int(np.argmax(bias_t))
        rew = bias_q[act] - d - (1 - term) * 0.5 * bias_t[sel]
        rew = np.where(knife, 0.0, rew)
        term = np.where(knife, 1, term).astype(np.int8)
        # knife-edge rows: tgt = 0 and pred = d needs bias_q[act] == d, which a constant head cannot give: those rows use d = +-1 instead
        d = np.where(knife, np.sign(d), d)
        rew = np.where(knife, bias_q[act] - d, rew)
        obs = rng.integers(0, 256, (n, 4, 1, 84, 84), dtype=np.uint8)
        nxt = rng.integers(0, 256, (n, 4, 1, 84, 84), dtype=np.uint8)
    batch = (obs, act.astype(np.int64), nxt, rew.astype(np.float32), term) + ((PER_W[b % 4].astype(np.float32),) if weighted else ())
    exact = ("q_pred_all", "q_next_all", "pred", "tgt") + (("td_errs",) if weighted else ())
    if mode == "zero" or kind == "cnn":
        exact = ("q_pred_all", "q_next_all", "pred", "tgt") if kind == "cnn" else ()
    zero = {}

    def coverage(r):
        if mode == "zero":
            return {"rows whose Q is the bias alone": ((r["q_pred_all"] == np.array([0.25, -0.5, 1.0])).all(1).sum(), n, False)}
        dd, tot = r["pred"] - r["tgt"], n
        cov = {}
        if d0_all:
            return {"d == 0": ((dd == 0).sum(), tot, False)}
        if weighted and clip is not None:
            a = np.abs(dd)
            cov.update({"|d| < cmin": ((a < clip[0]).sum(), tot, False), "|d| == cmin": ((a == clip[0]).sum(), tot, True), "inside": (((a > clip[0]) & (a < clip[1])).sum(), tot, True),
                        "|d| == cmax": ((a == clip[1]).sum(), tot, True), "|d| > cmax": ((a > clip[1]).sum(), tot, True), "d == 0": ((a == 0).sum(), tot, True)})
        else:
            a = np.abs(dd)
            cov.update({"|d| < 1": ((a < 1).sum(), tot, False), "|d| > 1": ((a > 1).sum(), tot, False), "|d| == 1": ((a == 1).sum(), tot, True), "d == 0": ((a == 0).sum(), tot, True)})
            if kind == "mlp" and dgrid is HUBER_D:
                cov.update({"|d| == 1 - 2^-24": ((a == 1 - E1).sum(), tot, True), "|d| == 1 + 2^-23": ((a == 1 + E2).sum(), tot, True), "|d| == 50": ((a == 50).sum(), tot, True)})
        if weighted:
            w = batch[5]
            cov.update({"w == 0": ((w == 0).sum(), tot, False), "w tiny": ((w == np.float32(1e-30)).sum(), tot, False), "w == 1": ((w == 1).sum(), tot, False),
                        "w large": ((w == 1e3).sum(), tot, False)})
        if ties and kind == "mlp":
            top2 = np.sort(nxt[:, :A].astype(np.float64), 1)[:, -2:]          # the online net's dialled next-state values select the action
            cov["rows with tied next-state maxima"] = ((top2[:, 0] == top2[:, 1]).sum(), tot, False)
        if all_term:
            cov["terminated"] = ((batch[4] == 1).sum(), tot, False)
        return cov
    return Case(name, "dqn", spec, (q, qt), [batch], branch, coverage, tuple(muts), exact, {}, zero,
                random_units="the online net's free hidden units (Mlp); the whole trunk (Nature-CNN, whose head has weight 0 and a dialled bias)")


# the one-workgroup step kernels take a batch of 32 at this shape, the layer-by-layer launches the batch of 250
DQN_PATHS = {32: {"lds_step": {}, "global_step": {"BDR_NO_MLP_LDS": "1"}, "layer_by_layer": {"BDR_NO_MLP_FUSED": "1"}},
             250: {"row_block_head": {"BDR_STEP_GRAPH": "0"}, "four_launches": {"BDR_STEP_GRAPH": "0", "BDR_NO_MLP_HEAD_FUSE": "1"}}}
DQN_ENV = ("BDR_NO_MLP_LDS", "BDR_NO_MLP_FUSED", "BDR_STEP_GRAPH", "BDR_NO_MLP_HEAD_FUSE", "BDR_NO_SMALL_GEMM")


def dqn_cases():
    clipm = ("clip_dropped", "clip_grad_open", "clip_grad_half_open", "clip_grad_open_interval")
    out = []
    for n in (32, 250):
        t = f"_b{n}"
        out += [
            dqn_case("huber_knife_edges" + t, "Huber quadratic / linear side with |d| in {0, 1 - 2^-24, 1, 1 + 2^-23, 50}", ("huber_quadratic", "huber_linear", "term_ignored", "relu0"), n=n),
            dqn_case("per_huber_clip" + t, "PER weights {0, 1e-30, 1, 1e3} and clip_td_err (0.25, 4) with |d| below, at, inside, at, above: the closed-range gradient mask",
                     clipm + ("weight_dropped", "huber_quadratic"), clip=CLIP, weighted=True, dgrid=CLIP_D, seed=1, n=n),
            dqn_case("per_mse_clip" + t, "the same through the MSE loss", clipm + ("weight_dropped",), clip=CLIP, weighted=True, dgrid=CLIP_D, loss="Mse", double_dqn=False, seed=2, n=n),
            dqn_case("per_d_zero" + t, "PER-weighted rows with d == 0 everywhere under clip_td_err: td = cmin, the loss is not 0, the gradient is exactly 0 (outside the clip, sgn(0) = 0)",
                     ("clip_dropped", "clip_grad_open+abs_grad1_at_0"), clip=CLIP, weighted=True, d0_all=True, seed=3, n=n),
            dqn_case("all_terminated" + t, "every row terminated: tgt = r", ("term_ignored",), all_term=True, seed=4, n=n),
            dqn_case("ddqn_argmax_ties" + t, "double-DQN with tied next-state maxima of the online net: the first index", ("argmax_last", "ddqn_dropped"), ties=True, seed=5, n=n),
            dqn_case("zero_networks" + t, "all weights 0: the loss comes from the biases, every hidden gradient is exactly 0", ("huber_quadratic",), mode="zero", seed=6, n=n),
            dqn_case("relu_at_zero" + t, "hidden pre-activations exactly 0: the dial units of Q column 0 in every row", ("relu0",), mode="relu0", seed=7, n=n),
        ]
    for arith in ("bf16x3_6", "f32_exact"):
        out.append(dqn_case(f"cnn_huber_{arith}", "Nature-CNN, head dialled through its bias: Huber sides and the kink, terminated rows, argmax ties of the target net",
                            ("huber_quadratic", "huber_linear", "term_ignored"), kind="cnn", n=16, double_dqn=False, ties=True, arithmetic=arith, dgrid=CNN_D, seed=8))
    out.append(dqn_case("cnn_per_clip_ddqn", "Nature-CNN, PER weights and clip_td_err, double DQN", clipm[:2] + ("weight_dropped",), kind="cnn", n=32, clip=CLIP, weighted=True,
                        dgrid=CLIP_D, seed=9))
    return out



# ======================================================================================================== IQN
@dataclass
class IqnSpec:
    in_dim: int = 6
    psi_units: Sequence[int] = (32,)
    feature_dim: int = 32
    embed_dim: int = 16
    f_units: Sequence[int] = (48,)
    n_actions: int = 4
    lr: float = 1e-4
    gamma: float = 0.5
    tau: float = 0.01

    def shapes3(self):
        return T.iqn_shapes("mlp", self.feature_dim, self.embed_dim, list(self.f_units), self.n_actions, psi_in=self.in_dim, psi_units=list(self.psi_units))

    def shapes(self):
        a, b, c = self.shapes3()
        return a + b + c

    def to_config(self, B, batch_size: int, **kw):
        f = B.MlpConfig(in_dim=self.in_dim, units=tuple(self.psi_units), out_dim=self.feature_dim, activation_out=True)
        return B.IqnConfig(f_config=f, feature_dim=self.feature_dim, embed_dim=self.embed_dim, m_units=tuple(self.f_units), n_actions=self.n_actions,
                           lr=self.lr, batch_size=batch_size, discount_factor=self.gamma, tau=self.tau, soft_update_interval=1, **kw)


class IqnRef:
    """Iqn::update_critic (iqn/base.rs:63-170, util/quantile_loss.rs:7-13) in float64 with given percent points"""

    def __init__(self, spec: IqnSpec, p, p_tgt, mut=(), dtype=DT):
        self.spec, self.mut, self.dtype = spec, frozenset(mut), dtype
        self.p = _unflat(p, spec.shapes(), dtype)
        self.p_tgt = _unflat(p_tgt, spec.shapes(), dtype, grad=False)
        self.n_psi = len(spec.shapes3()[0])
        self.st = dict(m=[torch.zeros_like(t) for t in self.p], v=[torch.zeros_like(t) for t in self.p], vmax=[torch.zeros_like(t) for t in self.p], step=0)

    def forward(self, p, x, tau):
        s = self.spec
        psi = _mlp(p[:self.n_psi], x, self.mut, relu_out=True)
        Bn, N = tau.shape
        i = torch.arange(1, s.embed_dim + 1, dtype=self.dtype).reshape(1, 1, -1)
        cos = torch.cos(tau.unsqueeze(-1) * (math.pi * i)).reshape(-1, s.embed_dim)
        relu = relu_grad1_at_0 if "relu0" in self.mut else torch.relu
        phi = relu(cos @ p[self.n_psi].T + p[self.n_psi + 1]).reshape(Bn, N, s.feature_dim)
        return _mlp(p[self.n_psi + 2:], psi.unsqueeze(1) * phi, self.mut)

    def update(self, obs, act, next_obs, reward, term, tau_pred, tau_tgt, terms=False) -> dict:
        s, mut = self.spec, self.mut
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32), dtype=self.dtype)
        obs, next_obs, reward, tau_p, tau_t = t(obs), t(next_obs), t(reward).unsqueeze(-1), t(tau_pred), t(tau_tgt)
        act = torch.as_tensor(np.asarray(act, np.int64)).reshape(-1, 1)
        not_term = t(1 - (0 * np.asarray(term) if "term_ignored" in mut else np.asarray(term))).unsqueeze(-1)
        n_p, n_t = tau_p.shape[1], tau_t.shape[1]
        z = self.forward(self.p, obs, tau_p)
        pred = z.gather(-1, act.unsqueeze(1).repeat(1, n_p, 1)).squeeze(-1).unsqueeze(1)            # [B, 1, Np]
        with torch.no_grad():
            zt = self.forward(self.p_tgt, next_obs, tau_t)
            a2 = zt.mean(1).argmax(-1).unsqueeze(-1).unsqueeze(-1).repeat(1, n_t, 1)
            tgt = (reward + not_term * f32(s.gamma) * zt.gather(2, a2).squeeze(-1)).unsqueeze(-1)    # [B, Nt, 1]
        diff = tgt - pred
        tau_rep = tau_p.unsqueeze(1).repeat(1, n_t, 1)
        if "tau_of_the_target" in mut:
            tau_rep = tau_t.unsqueeze(-1).repeat(1, 1, n_p)
        lt0 = (diff > 0) if "indicator_flipped" in mut else (diff < 0)
        wq = torch.full_like(diff, 0.5) if "quantile_weight_dropped" in mut else (tau_rep - lt0.to(diff.dtype)).abs()
        rows = (wq * smooth_l1_rows(diff, torch.zeros_like(diff), mut)).sum((1, 2)) / diff.numel()
        tm = {"grad": row_terms(rows, self.p)} if terms else {}
        for p in self.p:
            p.grad = None
        rows.sum().backward()
        out = dict(loss_critic=rows.sum(), terms_loss=rows, z_pred=z, z_tgt=zt, diff=diff, grad=_flat64(self.p, True))
        self.st["step"] += 1
        T.optimizer_step(self.p, self.st["m"], self.st["v"], self.st["vmax"], self.st["step"], s.lr, None)
        with torch.no_grad():
            for d, src in zip(self.p_tgt, self.p):
                d.copy_(f32(s.tau) * src + (1.0 - f32(s.tau)) * d)
        out.update(param=_flat64(self.p), param_tgt=_flat64(self.p_tgt))
        out = {k: (v.detach().numpy().astype(np.float64) if torch.is_tensor(v) else v) for k, v in out.items()}
        out["row_terms"] = tm
        return out


def iqn_f32(spec: IqnSpec, params, batches) -> dict:
    p, p_tgt = params
    r = T.TorchIqn("mlp", spec.shapes3(), p, lr=spec.lr, feature_dim=spec.feature_dim, embed_dim=spec.embed_dim, discount_factor=spec.gamma, tau=spec.tau,
                   soft_update_interval=1)
    r.p_tgt = T.unflatten(p_tgt, r.shapes)
    for b in batches:
        o = r.update(*b)
    return dict(loss_critic=o["loss"], z_pred=o["z_pred"], z_tgt=o["z_tgt"], grad=o["grads"], param=o["params"], param_tgt=o["tgt_params"])


# The merge net's last layer has weight 0 and a dialled bias: z[b, n, a] = bias[a] for every row and percent point, so d = tgt - pred is set
# per row through the reward (every pair of a row has the same d; a row with |d| > 1 has every pair on the linear side).  The feature
# net, the cosine embedding and the merge net's hidden layer stay random.
IQN_BIAS, IQN_BIAS_T = np.array([0.5, -1.0, 2.0, 0.0]), np.array([0.25, 1.5, 0.5, -2.0])
IQN_D = np.array([0, 0.5, -0.5, 1, -1, 0.25, 3, -3, 50, -50])


def iqn_case(name, branch, muts, *, n=60, n_p=9, n_t=5, big_reward=False, all_linear=False, seed=0, mode="dial"):
    """mode "dial": the constant head described above | "zero": every weight 0, every bias 0.5, the head's bias dialled | "relu0": a
    random network throughout (the gradient reaches every layer) in which four units of the feature net's output layer and four of the
    cosine embedding have weight and bias 0, so their pre-activation is exactly 0 in every row"""
    rng = np.random.default_rng(seed)
    spec = IqnSpec()
    A, shapes = spec.n_actions, spec.shapes()
    offs = np.concatenate([[0], np.cumsum([int(np.prod(sh)) for sh in shapes])])
    p = T.init_params(shapes, 17 + seed)
    nb = A * spec.f_units[-1] + A
    zero = {}
    if mode == "zero":
        for k, sh in enumerate(shapes):
            p[offs[k]:offs[k + 1]] = 0.0 if len(sh) == 2 else 0.5
    if mode == "relu0":
        k_psi, k_cos, Fd = len(spec.shapes3()[0]) - 2, len(spec.shapes3()[0]), spec.feature_dim
        idx = []
        for kw, rows in ((k_psi, range(0, 4)), (k_cos, range(4, 8))):
            width = shapes[kw][1]
            for r_ in rows:
                idx += list(range(offs[kw] + r_ * width, offs[kw] + (r_ + 1) * width)) + [offs[kw + 1] + r_]
        p[idx] = 0.0
        zero["grad"] = np.array(idx)      # relu'(0) = 0 decides these whole rows of two weight gradients (and their bias entries)
    else:
        p[-nb:] = np.concatenate([np.zeros(A * spec.f_units[-1]), IQN_BIAS]).astype(np.float32)
    pt = p.copy()
    if mode != "relu0":
        pt[-A:] = IQN_BIAS_T
    b = np.arange(n)
    act, term = b % A, (b % 3 == 0).astype(np.int8)
    d = IQN_D[b % len(IQN_D)]
    if all_linear:
        d = np.where(np.abs(d) > 1, d, np.where(b % 2 == 0, 2.0, -4.0))
    rew = IQN_BIAS[act] + d - (1 - term) * 0.5 * IQN_BIAS_T.max()
    if big_reward:
        rew = np.where(b % 2 == 0, 1e3, -1e3) + _q64(rng, n, -1, 1)
    obs, nxt = rng.standard_normal((n, spec.in_dim)).astype(np.float32), rng.standard_normal((n, spec.in_dim)).astype(np.float32)
    tau_p = np.tile(np.linspace(0, 1, n_p, dtype=np.float32), (n, 1))       # a Const grid that contains 0 and 1
    tau_t = np.tile(np.linspace(0, 1, n_t, dtype=np.float32), (n, 1))
    batch = (obs, act.astype(np.int64), nxt, rew.astype(np.float32), term, tau_p, tau_t)

    def coverage(r):
        dd = r["diff"]
        tot = dd.size
        ends = ((tau_p == 0) | (tau_p == 1)).sum() * n_t
        cov = {"d < 0": ((dd < 0).sum(), tot, False), "d > 0": ((dd > 0).sum(), tot, False), "tau == 0 or 1": (ends, tot, False)}
        if mode == "relu0":
            W = p[offs[k_psi]:offs[k_psi + 1]].reshape(shapes[k_psi])
            dead = ((W == 0).all(1) & (p[offs[k_psi + 1]:offs[k_psi + 2]] == 0)).sum()
            return {"(row, feature unit) pairs at pre-activation 0": (n * dead, n * Fd, True), "d < 0": cov["d < 0"], "d > 0": cov["d > 0"]}
        if mode == "zero":
            return {"rows whose z is the head's bias": ((r["z_pred"] == IQN_BIAS).all((1, 2)).sum(), n, False)}
        if big_reward:
            cov["|d| > 900"] = ((np.abs(dd) > 900).sum(), tot, False)
        elif all_linear:
            cov["rows with every pair on the linear side"] = ((np.abs(dd) > 1).all((1, 2)).sum(), n, False)
        else:
            cov.update({"|d| < 1": ((np.abs(dd) < 1).sum(), tot, False), "|d| > 1": ((np.abs(dd) > 1).sum(), tot, False), "|d| == 1": ((np.abs(dd) == 1).sum(), tot, True),
                        "d == 0": ((dd == 0).sum(), tot, True)})
        return cov
    return Case(name, "iqn", spec, (p, pt), [batch], branch, coverage, tuple(muts), ("z_pred", "z_tgt") if mode != "relu0" else (), {}, zero,
                random_units="every layer" if mode == "relu0" else "none" if mode == "zero" else"the feature net, the cosine embedding and the merge net's hidden layer; its last layer has weight 0 and a dialled bias")


def iqn_cases():
    return [
        iqn_case("huber_sides_const_grid", "pairwise quantile-Huber: d of both signs on both Huber sides, exactly 0 and exactly +-1; percent points 0 and 1; terminated rows",
                 ("indicator_flipped", "quantile_weight_dropped", "tau_of_the_target", "huber_quadratic", "huber_linear", "term_ignored")),
        iqn_case("all_pairs_linear", "every pair of every row on the linear side", ("huber_quadratic", "indicator_flipped"), all_linear=True, seed=1),
        iqn_case("rewards_1e3", "rewards of +-1e3: |d| about 1e3 on the linear side", ("huber_quadratic", "quantile_weight_dropped"), big_reward=True, seed=2),
        iqn_case("zero_networks", "all weights 0: the loss comes from the biases, every gradient behind the last layer is exactly 0", ("huber_quadratic",), mode="zero", seed=3),
        iqn_case("relu_at_zero", "a random network whose gradient reaches every layer; feature-net and cosine-embedding units at pre-activation exactly 0 in every row",
                 ("relu0", "indicator_flipped"), mode="relu0", seed=4),
    ]


CASES = {"iql": iql_cases, "awac": awac_cases, "bc": bc_cases, "sac": sac_cases, "dqn": dqn_cases, "iqn": iqn_cases}
