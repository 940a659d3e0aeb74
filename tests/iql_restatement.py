"""Independent restatement of border-candle-agent's Iql::opt_ (iql/base.rs:157-188) in float32 PyTorch autograd on the CPU: the checker
of the HIP IQL agent.  Nothing under border_amd/ imports this file.

  Linear        x @ W.T + b (candle_nn::Linear, weights [out][in]); Mlp: ReLU between layers, activation_out at the end (mlp.rs:14-24)
  update_value  q = min_i Qtgt_i(obs, act), u = q - V(obs), loss = mean(|tau - 1[u < 0]| u^2)           (:75-86, util.rs:262-266)
  update_critic tgt = r + gamma_not_done V'(next_obs), loss = mean_i mse|smooth_l1(Q_i, tgt), soft update (:88-121, util.rs:144-152, 235-255)
  update_actor  adv = min_i Qtgt_i(obs, act) - V'(obs), w = clamp(exp(inv_lambda adv), 0, max) | softmax, loss = mean(-logp w)  (:123-155)
  optimizers    Adam / AdamW element formulas (PyTorch's; candle-optimisers' Adam and candle-nn's AdamW compute the same quantities)

Parameters travel in the agent's reference layout: per layer ln{k}.weight [out][in] then ln{k}.bias [out]; the actor's mean Mlp
followed by head2 [act_dim].
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch


def mlp_shapes(in_dim: int, units: Sequence[int], out_dim: int):
    dims = [in_dim] + list(units) + [out_dim]
    return [((dims[k + 1], dims[k]), (dims[k + 1],)) for k in range(len(dims) - 1)]


def mlp_count(in_dim, units, out_dim) -> int:
    return sum(w[0] * w[1] + b[0] for w, b in mlp_shapes(in_dim, units, out_dim))


def init_flat(in_dim, units, out_dim, rng) -> np.ndarray:
    """uniform(+-1/sqrt(fan_in)) of every weight and bias, reference layout"""
    out = []
    for (o, i), _ in mlp_shapes(in_dim, units, out_dim):
        bd = 1.0 / math.sqrt(i)
        out.append(rng.uniform(-bd, bd, o * i)); out.append(rng.uniform(-bd, bd, o))
    return np.concatenate(out).astype(np.float32)


class Mlp:
    def __init__(self, in_dim, units, out_dim, relu_out: bool, flat: np.ndarray):
        self.shapes = mlp_shapes(in_dim, units, out_dim)
        self.relu_out = relu_out
        self.params: List[torch.Tensor] = []
        o = 0
        for ws, bs in self.shapes:
            for s in (ws, bs):
                n = int(np.prod(s))
                self.params.append(torch.tensor(np.asarray(flat[o:o + n], np.float32).reshape(s), requires_grad=True))
                o += n
        assert o == len(flat), (o, len(flat))

    def forward(self, x):
        n = len(self.params) // 2
        for k in range(n):
            x = x @ self.params[2 * k].T + self.params[2 * k + 1]
            if k < n - 1 or self.relu_out:
                x = torch.relu(x)
        return x

    def flat(self, grad=False) -> np.ndarray:
        return np.concatenate([(p.grad if grad else p).detach().numpy().reshape(-1) for p in self.params]).astype(np.float32)


class AdamState:
    """PyTorch's Adam / AdamW element formulas in f32 (border_amd's k_dense_reduce_adam computes the same quantities)."""

    def __init__(self, params, lr, adamw=False, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01):
        self.params, self.lr, self.adamw = params, lr, adamw
        self.b1, self.b2, self.eps, self.wd = (beta1, beta2, eps, wd) if adamw else (0.9, 0.999, 1e-8, 0.0)
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        for p, m, v in zip(self.params, self.m, self.v):
            g = p.grad
            p.mul_(np.float32(1 - self.lr * self.wd))
            m.mul_(self.b1).add_(g, alpha=1 - self.b1)
            v.mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
            denom = v.sqrt() / math.sqrt(bc2) + self.eps
            p.addcdiv_(m, denom, value=-(self.lr / bc1))


@dataclass
class IqlSpec:
    obs_dim: int
    act_dim: int
    v_units: Sequence[int] = (256, 256)
    p_units: Sequence[int] = (256, 256)
    q_units: Sequence[int] = (256, 256)
    n_critics: int = 2
    v_relu_out: bool = False
    q_relu_out: bool = False
    lr_value: float = 3e-4
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    adamw: dict = field(default_factory=dict)   # model name ("value" / "actor" / "critic") -> AdamW kwargs (beta1, beta2, eps, wd)
    critic_tau: float = 0.005
    gamma: float = 0.99
    tau_iql: float = 0.7
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
        return dict(actor=mlp_count(O, self.p_units, A) + A, critic=mlp_count(O + A, self.q_units, 1), value=mlp_count(O, self.v_units, 1))

    def init_params(self, seed: int):
        rng = np.random.default_rng(seed)
        O, A = self.obs_dim, self.act_dim
        actor = np.concatenate([init_flat(O, self.p_units, A, rng), rng.uniform(-0.5, 0.5, A).astype(np.float32)])
        critics = [init_flat(O + A, self.q_units, 1, rng) for _ in range(self.n_critics)]
        value = init_flat(O, self.v_units, 1, rng)
        return actor, critics, [c.copy() for c in critics], value

    def to_config(self, B, batch_size: int, **kw):
        """the border_amd.IqlConfig of this spec"""
        opt = lambda name, lr: (B.OptimizerConfig.AdamW(lr, **self.adamw[name]) if name in self.adamw else B.OptimizerConfig.Adam(lr))
        act = "ReLU"
        return B.IqlConfig(
            obs_dim=self.obs_dim, act_dim=self.act_dim,
            value_config=B.ValueConfig(B.CandleMlpConfig(tuple(self.v_units), act if self.v_relu_out else "None"), opt("value", self.lr_value)),
            critic_config=B.MultiCriticConfig(self.n_critics, B.CandleMlpConfig(tuple(self.q_units), act if self.q_relu_out else "None"),
                                              opt("critic", self.lr_critic), self.critic_tau),
            actor_config=B.GaussianActorConfig(B.CandleMlpConfig(tuple(self.p_units)), opt("actor", self.lr_actor), self.min_log_std, self.max_log_std,
                                               B.ActionLimit(self.action_limit, self.action_min, self.action_max, self.action_scale)),
            gamma=self.gamma, tau_iql=self.tau_iql, inv_lambda=self.inv_lambda, adv_softmax=self.adv_softmax, critic_loss=self.critic_loss,
            exp_adv_max=self.exp_adv_max, batch_size=batch_size, **kw)


def smooth_l1(x, y):
    d = (x - y).abs()
    m1 = (d < 1.0).float()
    return (0.5 * m1 * d ** 2 + (1.0 - m1) * (d - 0.5)).mean()


def normal_logp(x, mean, std):   # util/actor.rs:19-25
    var = std ** 2
    return (-0.5 * math.log(2 * math.pi) - 0.5 * var.log() - (0.5 / var) * (x - mean) ** 2).sum(-1)


def atanh_clamped(t):   # util.rs:268-271
    t = t.clamp(-0.999999, 0.999999)
    return 0.5 * ((1.0 + t) / (1.0 - t)).log()


class IqlRestatement:
    def __init__(self, spec: IqlSpec, actor, critics, critics_tgt, value):
        s = self.spec = spec
        O, A = s.obs_dim, s.act_dim
        self.actor = Mlp(O, s.p_units, A, False, actor[:-A])
        self.head2 = torch.tensor(np.asarray(actor[-A:], np.float32).reshape(1, A), requires_grad=True)
        self.critics = [Mlp(O + A, s.q_units, 1, s.q_relu_out, c) for c in critics]
        self.targets = [Mlp(O + A, s.q_units, 1, s.q_relu_out, c) for c in critics_tgt]
        self.value = Mlp(O, s.v_units, 1, s.v_relu_out, value)

        def opt(name, params, lr):
            kw = s.adamw.get(name)
            return AdamState(params, lr, adamw=kw is not None, **(kw or {}))
        self.opt_v = opt("value", self.value.params, s.lr_value)
        self.opt_q = opt("critic", [p for c in self.critics for p in c.params], s.lr_critic)
        self.opt_pi = opt("actor", self.actor.params + [self.head2], s.lr_actor)
        self.n_opts = 0

    # ---- helpers
    def q_tgt_min(self, obs, act):
        x = torch.cat([obs, act], 1)
        with torch.no_grad():
            return torch.stack([t.forward(x).squeeze(-1) for t in self.targets], 0).min(0).values

    def logp(self, obs, act):   # util/actor.rs:196-223
        s = self.spec
        mean = self.actor.forward(obs)
        lstd = self.head2.repeat(obs.shape[0], 1)
        std = lstd.clamp(s.min_log_std, s.max_log_std).exp()
        if s.action_limit == "Clamp":
            return normal_logp(act, mean, std)
        x = atanh_clamped(act / s.action_scale)
        a = act.clamp(-0.999999, 0.999999)
        lj = (-1.0 * (1.0 - a ** 2).log()).sum(-1)   # util.rs:274-279: the action itself, not act / scale
        return normal_logp(x, mean, std) + lj

    def sample(self, obs, z=None):
        """Policy::sample (util/actor.rs:226-241): z given = train mode"""
        s = self.spec
        with torch.no_grad():
            obs = torch.as_tensor(np.asarray(obs, np.float32))
            mean = self.actor.forward(obs)
            std = self.head2.clamp(s.min_log_std, s.max_log_std).exp()
            a = mean if z is None else std * torch.as_tensor(np.asarray(z, np.float32)) + mean
            a = a.clamp(s.action_min, s.action_max) if s.action_limit == "Clamp" else s.action_scale * a.tanh()
            return a.numpy()

    # ---- one Iql::opt_ loop iteration
    def update(self, obs, act, next_obs, reward, is_terminated, is_truncated) -> dict:
        s = self.spec
        t = lambda x: torch.as_tensor(np.asarray(x, np.float32))
        obs, act, next_obs, reward = t(obs), t(act), t(next_obs), t(reward).reshape(-1)
        done = (np.asarray(is_terminated, np.int8) | np.asarray(is_truncated, np.int8)).astype(np.float32)
        gnd = torch.as_tensor((np.float32(1.0) - done) * np.float32(s.gamma))   # util.rs:235-255, f32
        pr = {}
        # update_value
        for p in self.value.params:
            p.grad = None
        q = self.q_tgt_min(obs, act)
        v = self.value.forward(obs).squeeze(-1)
        u = q - v
        loss_value = ((s.tau_iql - (u < 0).float()).abs() * u ** 2).mean()
        loss_value.backward()
        pr.update(q_tgt_min_value=q.numpy().copy(), v=v.detach().numpy().copy(), u=u.detach().numpy().copy(), value_grad=self.value.flat(True))
        self.opt_v.step()
        # update_critic
        for c in self.critics:
            for p in c.params:
                p.grad = None
        x = torch.cat([obs, act], 1)
        preds = [c.forward(x).squeeze(-1) for c in self.critics]
        with torch.no_grad():
            v_next = self.value.forward(next_obs).squeeze(-1)
            tgt = reward + gnd * v_next
        losses = [((p - tgt) ** 2).mean() if s.critic_loss == "Mse" else smooth_l1(p, tgt) for p in preds]
        loss_critic = torch.stack(losses, 0).mean()
        loss_critic.backward()
        pr.update(tgt=tgt.numpy().copy(), v_next=v_next.numpy().copy(), q_pred=np.stack([p.detach().numpy() for p in preds]),
                  critic_grads=[c.flat(True) for c in self.critics])
        self.opt_q.step()
        with torch.no_grad():   # soft_update after every critic step (util/critic.rs:174-183, util.rs:51-71)
            for c, tc in zip(self.critics, self.targets):
                for p, tp in zip(c.params, tc.params):
                    tp.copy_(s.critic_tau * p + (1.0 - s.critic_tau) * tp)
        # update_actor
        for p in self.actor.params + [self.head2]:
            p.grad = None
        q3 = self.q_tgt_min(obs, act)
        with torch.no_grad():
            v_obs = self.value.forward(obs).squeeze(-1)
            adv = q3 - v_obs
            w = (adv * s.inv_lambda).exp().clamp(0.0, s.exp_adv_max) if not s.adv_softmax else torch.softmax(adv * s.inv_lambda, 0)
        logp = self.logp(obs, act)
        loss_actor = (-1.0 * logp * w).mean()
        loss_actor.backward()
        pr.update(q_tgt_min_actor=q3.numpy().copy(), v_obs=v_obs.numpy().copy(), w=w.numpy().copy(), logp=logp.detach().numpy().copy(),
                  actor_grad=np.concatenate([self.actor.flat(True), self.head2.grad.numpy().reshape(-1)]))
        self.opt_pi.step()
        self.n_opts += 1
        self.probes = pr
        return dict(loss_value=float(loss_value.detach()), loss_critic=float(loss_critic.detach()), loss_actor=float(loss_actor.detach()))

    # ---- parameters in the agent's reference layout
    def params(self, name: str) -> np.ndarray:
        if name == "actor":
            return np.concatenate([self.actor.flat(), self.head2.detach().numpy().reshape(-1)])
        if name == "value":
            return self.value.flat()
        if name.startswith("critic_tgt_"):
            return self.targets[int(name[len("critic_tgt_"):])].flat()
        return self.critics[int(name[len("critic_"):])].flat()


def make_batch(spec: IqlSpec, n: int, seed: int, p_done: float = 0.1):
    rng = np.random.default_rng(seed)
    O, A = spec.obs_dim, spec.act_dim
    obs = rng.standard_normal((n, O)).astype(np.float32)
    nxt = rng.standard_normal((n, O)).astype(np.float32)
    lo, hi = (spec.action_min, spec.action_max) if spec.action_limit == "Clamp" else (-0.9 * spec.action_scale, 0.9 * spec.action_scale)
    act = rng.uniform(lo, hi, (n, A)).astype(np.float32)
    rew = rng.standard_normal(n).astype(np.float32)
    term = (rng.random(n) < p_done).astype(np.int8)
    trunc = (rng.random(n) < p_done).astype(np.int8)
    return obs, act, nxt, rew, term, trunc
