"""Independent restatement of border-candle-agent's Sac::opt_ (sac/base.rs:124-134) in PyTorch autograd on the CPU: the checker of
the HIP candle SAC agent (float32; float64 for the error figures of tests/test_candle_sac_restatement.py).  Nothing under
border_amd/ imports this file.  The network, optimizer and log-likelihood pieces are those of tests/iql_restatement.py.

  actor         GaussianActor (util/actor.rs) over Mlp3 (mean Mlp + head2 [1, A]) or Mlp2 (mlp/mlp2.rs:33-44: trunk with ReLU after
                EVERY layer, mean = W_m h + b_m, second output exp(W_s h + b_s)); std = exp(clamp(second output))  (util/actor.rs:199-201)
  update_actor  a = actor.sample(obs) (not detached: z fixed, the gradient flows through a), logp = actor.logp(obs, a) on the limited
                action; EntCoef::update(logp.detach()) BEFORE alpha is read; q = min_i Q_i(obs, a) over the ONLINE critics with
                candle's reduce-min backward, an EQUALITY mask (every critic equal to the minimum receives the gradient);
                loss = mean(alpha logp - q)                                                                   (sac/base.rs:104-122)
  update_critic with the UPDATED actor and alpha: tgt = r + gnd (min_i Qtgt_i(next_obs, next_a) - alpha next_logp),
                gnd = (1 - is_terminated) gamma in f32 - is_truncated is ignored; loss = MEAN_i mse|smooth_l1(Q_i(obs, act), tgt);
                soft update of every target                                                                    (sac/base.rs:63-102, :132)
  EntCoef       Auto: loss = mean(-log_alpha (logp + target_entropy_f32)), one AdamW step (candle-nn defaults, wd 0.01);
                Fix(alpha): log_alpha = f32(ln alpha); alpha = exp(log_alpha)                                     (sac/ent_coef.rs)
  clamps        PyTorch's clamp passes the gradient on the closed range, bounds included: the project's recorded rule
                (tests/edge_inputs.py)

Policy::sample takes explicit N(0,1) draws z ([B][A], row-major); z = None is eval mode (the mean).
Actor parameters travel in the reference layout: Mlp3 as IQL's (mean Mlp, then head2); Mlp2: the trunk's ln{k}.weight / bias, then
mean.weight [A][H], mean.bias, std.weight, std.bias.

`mutate`: names of deliberate departures, for the mutation checks of tests/test_candle_sac_restatement.py.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np
import torch

from iql_restatement import AdamState, Mlp, atanh_clamped, init_flat, make_batch, mlp_count, normal_logp, smooth_l1  # noqa: F401

RECORD_KEYS = ("loss_critic", "loss_actor", "ent_coef")
MUTATIONS = ("jacobian_on_a_over_scale", "single_exp", "alpha_before_update", "target_with_old_actor", "sum_over_critics",
             "count_is_truncated", "argmin", "atanh_clamp_dropped")


class MinTie(torch.autograd.Function):
    """min over dim 0 whose backward is candle's: the output gradient goes to EVERY entry equal to the minimum"""

    @staticmethod
    def forward(ctx, qs):
        mn = qs.min(0).values
        ctx.save_for_backward(qs, mn)
        return mn

    @staticmethod
    def backward(ctx, g):
        qs, mn = ctx.saved_tensors
        return (qs == mn.unsqueeze(0)).to(qs.dtype) * g.unsqueeze(0)


@dataclass
class CandleSacSpec:
    obs_dim: int
    act_dim: int
    p_units: Sequence[int] = (256, 256)
    q_units: Sequence[int] = (256, 256)
    actor_kind: str = "Mlp2"
    n_critics: int = 2
    q_relu_out: bool = False
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    adamw: dict = field(default_factory=dict)   # "actor" / "critic" -> AdamW kwargs (beta1, beta2, eps, wd)
    critic_tau: float = 0.005
    gamma: float = 0.99
    ent_coef: tuple = ("Fix", 1.0)              # ("Fix", alpha) | ("Auto", target_entropy, lr)
    critic_loss: str = "Mse"
    min_log_std: float = -20.0
    max_log_std: float = 2.0
    action_limit: str = "Clamp"
    action_min: float = -1.0
    action_max: float = 1.0
    action_scale: float = 1.0

    def actor_count(self) -> int:
        O, A = self.obs_dim, self.act_dim
        if self.actor_kind == "Mlp3":
            return mlp_count(O, self.p_units, A) + A
        H = self.p_units[-1]
        return mlp_count(O, self.p_units[:-1], H) + 2 * (A * H + A)

    def init_params(self, seed: int, s_bias: float = -1.0):
        """(actor, critics, targets).  Mlp2's std.bias is shifted by s_bias so that exp(s) starts inside the log-std range more often"""
        rng = np.random.default_rng(seed)
        O, A = self.obs_dim, self.act_dim
        if self.actor_kind == "Mlp3":
            actor = np.concatenate([init_flat(O, self.p_units, A, rng), rng.uniform(-0.5, 0.5, A).astype(np.float32)])
        else:
            H = self.p_units[-1]
            bd = 1.0 / math.sqrt(H)
            heads = [rng.uniform(-bd, bd, n).astype(np.float32) for n in (A * H, A, A * H, A)]
            heads[3] = heads[3] + np.float32(s_bias)
            actor = np.concatenate([init_flat(O, self.p_units[:-1], H, rng)] + heads)
        critics = [init_flat(O + A, self.q_units, 1, rng) for _ in range(self.n_critics)]
        return actor, critics, [c.copy() for c in critics]

    def draws(self, n: int, seed: int, scale: float = 1.0):
        """(z_pi, z_next): the draws of a and next_a, [n][act_dim] each.  scale < 1 keeps u = mean + std z where a Tanh limit is
        not saturated (Mlp2's std is at least 1 with the default bounds): the host may hand the agent any draws"""
        rng = np.random.default_rng(seed)
        f = lambda: (scale * rng.standard_normal((n, self.act_dim))).astype(np.float32)
        return f(), f()

    def to_config(self, B, batch_size: int, **kw):
        """the border_amd.CandleSacConfig of this spec"""
        opt = lambda name, lr: (B.OptimizerConfig.AdamW(lr, **self.adamw[name]) if name in self.adamw else B.OptimizerConfig.Adam(lr))
        ent = B.EntCoefMode.Fix(self.ent_coef[1]) if self.ent_coef[0] == "Fix" else B.EntCoefMode.Auto(self.ent_coef[1], self.ent_coef[2])
        return B.CandleSacConfig(
            obs_dim=self.obs_dim, act_dim=self.act_dim,
            critic_config=B.MultiCriticConfig(self.n_critics, B.CandleMlpConfig(tuple(self.q_units), "ReLU" if self.q_relu_out else "None"),
                                              opt("critic", self.lr_critic), self.critic_tau),
            actor_config=B.GaussianActorConfig(B.CandleMlpConfig(tuple(self.p_units)), opt("actor", self.lr_actor), self.min_log_std, self.max_log_std,
                                               B.ActionLimit(self.action_limit, self.action_min, self.action_max, self.action_scale), kind=self.actor_kind),
            gamma=self.gamma, ent_coef_mode=ent, critic_loss=self.critic_loss, batch_size=batch_size, **kw)


def _cast(net: Mlp, dtype):
    net.params = [p.detach().to(dtype).requires_grad_() for p in net.params]
    return net


def _flat(params, grad=False) -> np.ndarray:
    return np.concatenate([(p.grad if grad else p).detach().numpy().reshape(-1) for p in params])


class TanhGiven(torch.autograd.Function):
    """tanh whose VALUES are handed in (the device's own tanhf, tests/test_gpu_candle_sac_edges.py) and whose derivative is
    1 - value^2: near saturation one float32 ulp of tanh moves 1 - tanh^2 by percents, which is not what those tests are about"""

    @staticmethod
    def forward(ctx, u, th):
        ctx.save_for_backward(th)
        return th.clone()

    @staticmethod
    def backward(ctx, g):
        (th,) = ctx.saved_tensors
        return g * (1.0 - th ** 2), None


class CandleSacRestatement:
    def __init__(self, spec: CandleSacSpec, actor, critics, critics_tgt, dtype=torch.float32, mutate=(), clamp1=0.999999, tanh_given=None):
        """clamp1: the bound of atanh's and the Jacobian's clamp (a float64 run that keeps the reference's float32 constant passes
        float(np.float32(0.999999))); tanh_given: [values for a, values for next_a] used in place of tanh(u), see TanhGiven"""
        s = self.spec = spec
        self.clamp1, self.tanh_given, self._tanh_call = clamp1, tanh_given, 0
        assert all(m in MUTATIONS for m in mutate), mutate
        self.mutate, self.dtype = set(mutate), dtype
        O, A = s.obs_dim, s.act_dim
        actor = np.asarray(actor, np.float32)
        assert actor.size == s.actor_count()
        leaf = lambda x, shape: torch.tensor(np.asarray(x, np.float32).reshape(shape)).to(dtype).requires_grad_()
        if s.actor_kind == "Mlp3":
            self.trunk = _cast(Mlp(O, s.p_units, A, False, actor[:-A]), dtype)
            self.heads = [leaf(actor[-A:], (1, A))]
        else:
            assert len(s.p_units) >= 2   # mlp.rs:14-24: the loop bound underflows with one trunk layer
            H = s.p_units[-1]
            nt = mlp_count(O, s.p_units[:-1], H)
            self.trunk = _cast(Mlp(O, s.p_units[:-1], H, True, actor[:nt]), dtype)   # ReLU after the last trunk layer too
            o, self.heads = nt, []
            for shape in ((A, H), (A,), (A, H), (A,)):   # mean.weight, mean.bias, std.weight, std.bias
                n = int(np.prod(shape))
                self.heads.append(leaf(actor[o:o + n], shape)); o += n
        self.actor_params = self.trunk.params + self.heads
        self.critics = [_cast(Mlp(O + A, s.q_units, 1, s.q_relu_out, c), dtype) for c in critics]
        self.targets = [_cast(Mlp(O + A, s.q_units, 1, s.q_relu_out, c), dtype) for c in critics_tgt]

        def opt(name, params, lr):
            kw = s.adamw.get(name)
            return AdamState(params, lr, adamw=kw is not None, **(kw or {}))
        self.opt_q = opt("critic", [p for c in self.critics for p in c.params], s.lr_critic)
        self.opt_pi = opt("actor", self.actor_params, s.lr_actor)
        # EntCoef::new (ent_coef.rs:30-56)
        la = np.float32(math.log(s.ent_coef[1])) if s.ent_coef[0] == "Fix" else np.float32(0.0)
        self.log_alpha = torch.tensor([la]).to(dtype).requires_grad_()
        self.opt_alpha = AdamState([self.log_alpha], s.ent_coef[2], adamw=True) if s.ent_coef[0] == "Auto" else None
        self.n_opts = 0

    # ---- the actor
    def dist(self, obs):
        """(mean, second output) of the policy model"""
        h = self.trunk.forward(obs)
        if self.spec.actor_kind == "Mlp3":
            return h, self.heads[0].repeat(obs.shape[0], 1)
        wm, bm, ws, bs = self.heads
        sv = h @ ws.T + bs
        return h @ wm.T + bm, (sv if "single_exp" in self.mutate else sv.exp())

    def sample_logp(self, obs, z):
        """a = actor.sample(obs), logp = actor.logp(obs, a): the second forward of logp has the same bits, so one serves both"""
        s = self.spec
        mean, l = self.dist(obs)
        std = l.clamp(s.min_log_std, s.max_log_std).exp()
        u = mean if z is None else std * z + mean
        if s.action_limit == "Clamp":
            a = u.clamp(s.action_min, s.action_max)
            return a, normal_logp(a, mean, std)
        if self.tanh_given is None:
            th = u.tanh()
        else:
            th = TanhGiven.apply(u, torch.as_tensor(np.asarray(self.tanh_given[self._tanh_call % 2])).to(self.dtype))
            self._tanh_call += 1
        a = s.action_scale * th
        r = a / s.action_scale
        c1 = self.clamp1
        if "atanh_clamp_dropped" in self.mutate:
            x = 0.5 * ((1.0 + r) / (1.0 - r)).log()
        elif c1 == 0.999999:
            x = atanh_clamped(r)
        else:
            rc = r.clamp(-c1, c1)
            x = 0.5 * ((1.0 + rc) / (1.0 - rc)).log()
        ac = (r if "jacobian_on_a_over_scale" in self.mutate else a).clamp(-c1, c1)   # util.rs:274-279: the action itself
        lj = (-1.0 * (1.0 - ac ** 2).log()).sum(-1)
        return a, normal_logp(x, mean, std) + lj

    def sample(self, obs, z=None) -> np.ndarray:
        """Policy::sample (util/actor.rs:226-241): z given = train mode (mean + std z), None = eval mode (mean)"""
        with torch.no_grad():
            obs = torch.as_tensor(np.asarray(obs, np.float32)).to(self.dtype)
            z = None if z is None else torch.as_tensor(np.asarray(z, np.float32)).to(self.dtype)
            return self.sample_logp(obs, z)[0].numpy()

    def alpha(self):
        return self.log_alpha.detach().exp()

    # ---- one Sac::opt_ loop iteration
    def update(self, obs, act, next_obs, reward, is_terminated, is_truncated, z_pi=None, z_next=None) -> dict:
        """z_pi / z_next: the draws of a and next_a (train mode); None for both = eval mode."""
        s, mu = self.spec, self.mutate
        t = lambda x: None if x is None else torch.as_tensor(np.asarray(x, np.float32)).to(self.dtype)
        obs, act, next_obs, reward, z_pi, z_next = t(obs), t(act), t(next_obs), t(reward).reshape(-1), t(z_pi), t(z_next)
        done = np.asarray(is_terminated, np.int8)
        if "count_is_truncated" in mu:
            done = done | np.asarray(is_truncated, np.int8)
        gnd = torch.as_tensor((np.float32(1.0) - done.astype(np.float32)) * np.float32(s.gamma)).to(self.dtype)   # util.rs:235-255, f32
        pr = {}
        # ---------------- update_actor (:104-122)
        for p in self.actor_params:
            p.grad = None
        a, logp = self.sample_logp(obs, z_pi)
        alpha_old = self.alpha()
        if self.opt_alpha is not None:   # EntCoef::update(logp.detach()) (ent_coef.rs:71-84)
            te = torch.tensor(np.float32(s.ent_coef[1])).to(self.dtype)
            self.log_alpha.grad = None
            (-1.0 * self.log_alpha * (logp.detach() + te)).mean(0).sum().backward()
            pr["log_alpha_grad"] = self.log_alpha.grad.numpy().copy()
            self.opt_alpha.step()
        alpha = alpha_old if "alpha_before_update" in mu else self.alpha()
        x = torch.cat([obs, a], 1)
        qs = torch.stack([c.forward(x).squeeze(-1) for c in self.critics], 0)
        q = qs.min(0).values if "argmin" in mu else MinTie.apply(qs)
        pr["dq_da"] = torch.autograd.grad(q.sum(), a, retain_graph=True)[0].numpy().copy()
        loss_actor = (alpha * logp - q).mean()
        grads = torch.autograd.grad(loss_actor, self.actor_params)   # the critics receive no step from this loss
        for p, g in zip(self.actor_params, grads):
            p.grad = g
        pr.update(a=a.detach().numpy().copy(), logp=logp.detach().numpy().copy(), q_min=q.detach().numpy().copy(),
                  actor_grad=_flat(self.actor_params, True))
        if "target_with_old_actor" in mu:
            with torch.no_grad():
                old_next = self.sample_logp(next_obs, z_next)
        self.opt_pi.step()
        # ---------------- update_critic (:63-102), next_a from the actor just updated
        for c in self.critics:
            for p in c.params:
                p.grad = None
        x = torch.cat([obs, act], 1)
        preds = [c.forward(x).squeeze(-1) for c in self.critics]
        with torch.no_grad():
            next_a, next_logp = old_next if "target_with_old_actor" in mu else self.sample_logp(next_obs, z_next)
            xn = torch.cat([next_obs, next_a], 1)
            next_q = torch.stack([n.forward(xn).squeeze(-1) for n in self.targets], 0).min(0).values
            next_q = next_q - alpha * next_logp
            tgt = reward + gnd * next_q
        losses = [((p - tgt) ** 2).mean() if s.critic_loss == "Mse" else smooth_l1(p, tgt) for p in preds]
        loss_critic = torch.stack(losses, 0).sum() if "sum_over_critics" in mu else torch.stack(losses, 0).mean()
        loss_critic.backward()
        pr.update(next_a=next_a.numpy().copy(), next_logp=next_logp.numpy().copy(), tgt=tgt.numpy().copy(),
                  q_pred=np.stack([p.detach().numpy() for p in preds]), critic_grads=[_flat(c.params, True) for c in self.critics])
        self.opt_q.step()
        with torch.no_grad():   # soft_update (sac/base.rs:132; util/critic.rs:174-183)
            for c, tc in zip(self.critics, self.targets):
                for p, tp in zip(c.params, tc.params):
                    tp.copy_(s.critic_tau * p + (1.0 - s.critic_tau) * tp)
        self.n_opts += 1
        self.probes = pr
        return dict(loss_critic=float(loss_critic.detach()), loss_actor=float(loss_actor.detach()), ent_coef=float(self.alpha()))

    def opt_record(self, recs) -> dict:
        """the Record of one opt_ (:136-146): f32 sums of the two losses divided by the update count; alpha after the last update"""
        n = np.float32(len(recs))
        out = {}
        for k in ("loss_critic", "loss_actor"):
            acc = np.float32(0)
            for r in recs:
                acc = np.float32(acc + np.float32(r[k]))
            out[k] = float(acc / n)
        out["ent_coef"] = recs[-1]["ent_coef"]
        return out

    # ---- parameters in the agent's reference layout
    def params(self, name: str) -> np.ndarray:
        if name == "actor":
            return _flat(self.actor_params)
        if name == "log_alpha":
            return self.log_alpha.detach().numpy().copy()
        if name.startswith("critic_tgt_"):
            return _flat(self.targets[int(name[len("critic_tgt_"):])].params)
        return _flat(self.critics[int(name[len("critic_"):])].params)


def rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


FIGURE_KEYS = ("actor_grad", "critic_grad", "a", "logp", "q_min", "dq_da", "next_a", "next_logp", "tgt", "q_pred", "actor", "critic")


def f32_f64_figures(r32: CandleSacRestatement, r64: CandleSacRestatement) -> dict:
    """After the same update on a float32 and a float64 restatement: how far float32 arithmetic alone moves each compared quantity.
    Max-relative for gradients and probes, max-absolute for the parameters (`actor`, `critic`)."""
    p, q = r32.probes, r64.probes
    nc = r32.spec.n_critics
    out = {k: rel(p[k], q[k]) for k in ("actor_grad", "a", "logp", "q_min", "dq_da", "next_a", "next_logp", "tgt", "q_pred")}
    out["critic_grad"] = max(rel(p["critic_grads"][i], q["critic_grads"][i]) for i in range(nc))
    out["actor"] = float(np.abs(r32.params("actor") - r64.params("actor")).max())
    out["critic"] = max(float(np.abs(r32.params(f"critic_{i}") - r64.params(f"critic_{i}")).max()) for i in range(nc))
    return out
