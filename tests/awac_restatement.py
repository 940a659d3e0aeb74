"""Independent restatement of border-candle-agent's Awac::opt_ (awac/base.rs:170-215) in float32 PyTorch autograd on the CPU: the
checker of the HIP AWAC agent.  Nothing under border_amd/ imports this file.  The network, optimizer and log-likelihood pieces are
those of tests/iql_restatement.py (the same GaussianActor and MultiCritic).

  update_actor  act_ = actor.sample(obs), q = min_i Q_i(obs, act), v = min_i Q_i(obs, act_) (ONLINE critics, util/critic.rs:197-202),
                adv = q - v, w = clamp(exp(inv_lambda adv), 0, max) | softmax, loss = mean(-logp(act | obs) w)        (:127-168)
  update_critic next_act = actor.sample(next_obs) of the UPDATED actor, tgt = r + gamma_not_done min_i Qtgt_i(next_obs, next_act),
                loss = SUM_i mse|smooth_l1(Q_i(obs, act), tgt), soft update of every target              (:66-125, util.rs:235-255)
  opt_          per update: update_actor, then update_critic on the same batch; the record's first five values are averaged over
                the updates, logp_mean, reward_mean and next_q_mean summed                                       (:170-215)

Policy::sample (util/actor.rs:226-241) takes explicit N(0,1) draws z ([B][A], row-major); z = None is eval mode (the mean).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Sequence

import numpy as np
import torch

from iql_restatement import AdamState, Mlp, atanh_clamped, init_flat, make_batch, mlp_count, normal_logp, smooth_l1  # noqa: F401

RECORD_KEYS = ("loss_critic", "loss_actor", "q_tgt_abs_mean", "adv_mean", "adv_abs_mean", "logp_mean", "reward_mean", "next_q_mean")


@dataclass
class AwacSpec:
    obs_dim: int
    act_dim: int
    p_units: Sequence[int] = (256, 256)
    q_units: Sequence[int] = (256, 256)
    n_critics: int = 2
    q_relu_out: bool = False
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    adamw: dict = field(default_factory=dict)   # "actor" / "critic" -> AdamW kwargs (beta1, beta2, eps, wd)
    critic_tau: float = 0.005
    gamma: float = 0.99
    inv_lambda: float = 10.0
    exp_adv_max: float = 100.0
    adv_softmax: bool = False
    critic_loss: str = "Mse"
    min_log_std: float = -20.0
    max_log_std: float = 2.0
    action_limit: str = "Clamp"
    action_min: float = -1.0
    action_max: float = 1.0
    action_scale: float = 1.0

    def counts(self):
        O, A = self.obs_dim, self.act_dim
        return dict(actor=mlp_count(O, self.p_units, A) + A, critic=mlp_count(O + A, self.q_units, 1))

    def init_params(self, seed: int):
        rng = np.random.default_rng(seed)
        O, A = self.obs_dim, self.act_dim
        actor = np.concatenate([init_flat(O, self.p_units, A, rng), rng.uniform(-0.5, 0.5, A).astype(np.float32)])
        critics = [init_flat(O + A, self.q_units, 1, rng) for _ in range(self.n_critics)]
        return actor, critics, [c.copy() for c in critics]

    def draws(self, n: int, seed: int):
        """(z_pi, z_next): the N(0,1) draws of act_ and next_act, [n][act_dim] each"""
        rng = np.random.default_rng(seed)
        return (rng.standard_normal((n, self.act_dim)).astype(np.float32), rng.standard_normal((n, self.act_dim)).astype(np.float32))

    def to_config(self, B, batch_size: int, **kw):
        """the border_amd.AwacConfig of this spec"""
        opt = lambda name, lr: (B.OptimizerConfig.AdamW(lr, **self.adamw[name]) if name in self.adamw else B.OptimizerConfig.Adam(lr))
        return B.AwacConfig(
            obs_dim=self.obs_dim, act_dim=self.act_dim,
            critic_config=B.MultiCriticConfig(self.n_critics, B.CandleMlpConfig(tuple(self.q_units), "ReLU" if self.q_relu_out else "None"),
                                              opt("critic", self.lr_critic), self.critic_tau),
            actor_config=B.GaussianActorConfig(B.CandleMlpConfig(tuple(self.p_units)), opt("actor", self.lr_actor), self.min_log_std, self.max_log_std,
                                               B.ActionLimit(self.action_limit, self.action_min, self.action_max, self.action_scale)),
            gamma=self.gamma, inv_lambda=self.inv_lambda, adv_softmax=self.adv_softmax, critic_loss=self.critic_loss,
            exp_adv_max=self.exp_adv_max, batch_size=batch_size, **kw)


class AwacRestatement:
    def __init__(self, spec: AwacSpec, actor, critics, critics_tgt):
        s = self.spec = spec
        O, A = s.obs_dim, s.act_dim
        self.actor = Mlp(O, s.p_units, A, False, actor[:-A])
        self.head2 = torch.tensor(np.asarray(actor[-A:], np.float32).reshape(1, A), requires_grad=True)
        self.critics = [Mlp(O + A, s.q_units, 1, s.q_relu_out, c) for c in critics]
        self.targets = [Mlp(O + A, s.q_units, 1, s.q_relu_out, c) for c in critics_tgt]

        def opt(name, params, lr):
            kw = s.adamw.get(name)
            return AdamState(params, lr, adamw=kw is not None, **(kw or {}))
        self.opt_q = opt("critic", [p for c in self.critics for p in c.params], s.lr_critic)
        self.opt_pi = opt("actor", self.actor.params + [self.head2], s.lr_actor)
        self.n_opts = 0

    # ---- helpers
    @staticmethod
    def q_min(nets, obs, act):   # util/critic.rs:197-218: min over the critics of Q_i(obs, act)
        x = torch.cat([obs, act], 1)
        with torch.no_grad():
            return torch.stack([n.forward(x).squeeze(-1) for n in nets], 0).min(0).values

    def logp(self, obs, act):   # util/actor.rs:196-223
        s = self.spec
        mean = self.actor.forward(obs)
        std = self.head2.repeat(obs.shape[0], 1).clamp(s.min_log_std, s.max_log_std).exp()
        if s.action_limit == "Clamp":
            return normal_logp(act, mean, std)
        x = atanh_clamped(act / s.action_scale)
        a = act.clamp(-0.999999, 0.999999)
        lj = (-1.0 * (1.0 - a ** 2).log()).sum(-1)   # util.rs:274-279: the action itself, not act / scale
        return normal_logp(x, mean, std) + lj

    def sample(self, obs, z=None):
        """Policy::sample (util/actor.rs:226-241): z given = train mode (mean + std z), None = eval mode (mean)"""
        s = self.spec
        with torch.no_grad():
            obs = torch.as_tensor(np.asarray(obs, np.float32))
            mean = self.actor.forward(obs)
            std = self.head2.clamp(s.min_log_std, s.max_log_std).exp()
            a = mean if z is None else std * torch.as_tensor(np.asarray(z, np.float32)) + mean
            a = a.clamp(s.action_min, s.action_max) if s.action_limit == "Clamp" else s.action_scale * a.tanh()
            return a

    # ---- one Awac::opt_ loop iteration
    def update(self, obs, act, next_obs, reward, is_terminated, is_truncated, z_pi=None, z_next=None) -> dict:
        """z_pi / z_next: the draws of act_ and next_act (train mode); None for both = eval mode."""
        s = self.spec
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32))
        obs, act, next_obs, reward = t(obs), t(act), t(next_obs), t(reward).reshape(-1)
        done = (np.asarray(is_terminated, np.int8) | np.asarray(is_truncated, np.int8)).astype(np.float32)
        gnd = torch.as_tensor((np.float32(1.0) - done) * np.float32(s.gamma))   # util.rs:235-255, f32
        pr = {}
        # update_actor (:127-168)
        for p in self.actor.params + [self.head2]:
            p.grad = None
        act_ = self.sample(obs, z_pi)
        q = self.q_min(self.critics, obs, act)
        v = self.q_min(self.critics, obs, act_)
        adv = q - v
        with torch.no_grad():
            w = (adv * s.inv_lambda).exp().clamp(0.0, s.exp_adv_max) if not s.adv_softmax else torch.softmax(adv * s.inv_lambda, 0)
        logp = self.logp(obs, act)
        loss_actor = (-1.0 * logp * w).mean()
        loss_actor.backward()
        pr.update(q_data_min=q.numpy().copy(), q_pi_min=v.numpy().copy(), adv=adv.numpy().copy(), w=w.numpy().copy(),
                  logp=logp.detach().numpy().copy(), act_=act_.numpy().copy(),
                  actor_grad=np.concatenate([self.actor.flat(True), self.head2.grad.numpy().reshape(-1)]))
        self.opt_pi.step()
        rec = dict(loss_actor=float(loss_actor.detach()), adv_mean=float(adv.mean()), adv_abs_mean=float(adv.abs().mean()),
                   logp_mean=float(logp.detach().mean()))
        # update_critic (:66-125), next_act from the actor just updated
        for c in self.critics:
            for p in c.params:
                p.grad = None
        x = torch.cat([obs, act], 1)
        preds = [c.forward(x).squeeze(-1) for c in self.critics]
        next_act = self.sample(next_obs, z_next)
        next_q = self.q_min(self.targets, next_obs, next_act)
        tgt = reward + gnd * next_q
        losses = [((p - tgt) ** 2).mean() if s.critic_loss == "Mse" else smooth_l1(p, tgt) for p in preds]
        loss_critic = torch.stack(losses, 0).sum()
        loss_critic.backward()
        pr.update(next_act=next_act.numpy().copy(), next_q=next_q.numpy().copy(), tgt=tgt.numpy().copy(),
                  q_pred=np.stack([p.detach().numpy() for p in preds]), critic_grads=[c.flat(True) for c in self.critics])
        self.opt_q.step()
        with torch.no_grad():   # soft_update after every critic step (util/critic.rs:174-183, util.rs:51-71)
            for c, tc in zip(self.critics, self.targets):
                for p, tp in zip(c.params, tc.params):
                    tp.copy_(s.critic_tau * p + (1.0 - s.critic_tau) * tp)
        rec.update(loss_critic=float(loss_critic.detach()), q_tgt_abs_mean=float(tgt.abs().mean()), reward_mean=float(reward.mean()),
                   next_q_mean=float(next_q.mean()))
        self.n_opts += 1
        self.probes = pr
        return {k: rec[k] for k in RECORD_KEYS}

    def opt_record(self, recs) -> dict:
        """the Record of one opt_ from the per-update records (:197-212): f32 sums, the first five divided by the update count"""
        out = {}
        n = np.float32(len(recs))
        for i, k in enumerate(RECORD_KEYS):
            acc = np.float32(0)
            for r in recs:
                acc = np.float32(acc + np.float32(r[k]))
            out[k] = float(acc / n) if i < 5 else float(acc)
        return out

    # ---- parameters in the agent's reference layout
    def params(self, name: str) -> np.ndarray:
        if name == "actor":
            return np.concatenate([self.actor.flat(), self.head2.detach().numpy().reshape(-1)])
        if name.startswith("critic_tgt_"):
            return self.targets[int(name[len("critic_tgt_"):])].flat()
        return self.critics[int(name[len("critic_"):])].flat()
