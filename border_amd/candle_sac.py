"""Host-side mirror of border-candle-agent's Sac agent over the C ABI (online RL).  Not border_amd.sac, which mirrors
border-tch-agent's SAC.

  CandleSacConfig  border-candle-agent/src/sac/config.rs (defaults :82-93): actor_config, critic_config, gamma, ent_coef_mode,
                   n_updates_per_opt, batch_size, critic_loss, device.  No reward_scale, no log-std bounds of its own.
  EntCoefMode      sac/ent_coef.rs:13-19: Fix(alpha) | Auto(target_entropy, learning_rate)
  CandleSac        sac/base.rs (Agent, Policy::sample; SyncModel ships the actor, as for IQL and AWAC)

The model configs are IQL's (border_amd.iql).  GaussianActorConfig.kind chooses the policy model: "Mlp3" (mlp/mlp3.rs) or "Mlp2"
(mlp/mlp2.rs, what the reference's SAC examples build); only this config reads it.
batch_size must be >= 2 (include/border_amd.h says why the reference cannot run a one-row batch).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from .iql import CandleAgent, GaussianActorConfig, MultiCriticConfig, _p

RECORD_KEYS = ("loss_critic", "loss_actor", "ent_coef")
ACTOR_KINDS = {"Mlp3": 0, "Mlp2": 1}   # BDR_ACTOR_*


@dataclass
class EntCoefMode:
    kind: str = "Fix"            # "Fix" | "Auto"
    alpha: float = 1.0           # Fix(alpha)
    target_entropy: float = 0.0  # Auto(target_entropy, lr)
    lr: float = 3e-4

    @classmethod
    def Fix(cls, alpha: float) -> "EntCoefMode":
        return cls("Fix", alpha=alpha)

    @classmethod
    def Auto(cls, target_entropy: float, lr: float) -> "EntCoefMode":
        return cls("Auto", target_entropy=target_entropy, lr=lr)


@dataclass
class CandleSacConfig:
    obs_dim: int = 0
    act_dim: int = 0
    actor_config: GaussianActorConfig = field(default_factory=GaussianActorConfig)
    critic_config: MultiCriticConfig = field(default_factory=MultiCriticConfig)
    gamma: float = 0.99
    ent_coef_mode: EntCoefMode = field(default_factory=lambda: EntCoefMode.Fix(1.0))
    n_updates_per_opt: int = 1
    batch_size: int = 1
    critic_loss: str = "Mse"
    train: bool = False
    seed: int = 0
    device: Optional[int] = None

    def to_c(self) -> _lib.CandleSacConfigC:
        c = _lib.CandleSacConfigC()
        _lib.lib().bdr_candle_sac_config_default(C.byref(c))
        c.obs_dim, c.act_dim = self.obs_dim, self.act_dim
        self.actor_config.policy_config.fill(c.actor)
        self.critic_config.q_config.fill(c.critic)
        c.n_critics, c.critic_tau = self.critic_config.n_nets, self.critic_config.tau
        for name, o in (("actor", self.actor_config.opt_config), ("critic", self.critic_config.opt_config)):
            setattr(c, "lr_" + name, o.lr)
            getattr(c, "opt_" + name).fill(o)
        ac = self.actor_config
        c.actor_kind = ACTOR_KINDS[ac.kind]
        c.min_log_std, c.max_log_std = ac.min_log_std, ac.max_log_std
        lim = ac.action_limit
        c.action_limit = {"Clamp": 0, "Tanh": 1}[lim.kind]
        c.action_min, c.action_max, c.action_scale = lim.action_min, lim.action_max, lim.action_scale
        c.gamma = self.gamma
        e = self.ent_coef_mode
        c.ent_coef_mode = {"Fix": 0, "Auto": 1}[e.kind]
        c.ent_coef_alpha, c.target_entropy, c.ent_coef_lr = e.alpha, e.target_entropy, e.lr
        c.critic_loss = {"Mse": 0, "SmoothL1": 1}[self.critic_loss]
        c.n_updates_per_opt, c.batch_size, c.train, c.seed = self.n_updates_per_opt, self.batch_size, int(self.train), self.seed
        c.device = -1 if self.device is None else self.device
        return c


class CandleSac(CandleAgent):
    """sac/base.rs; checkpoints (sac/base.rs:244-270): actor, critic, critic.tgt, ent_coef."""
    KIND = "candle_sac"
    CKPT_STEMS = ("actor", "critic", "critic.tgt", "ent_coef")

    def _model_id(self, name: str) -> int:
        return 1 + 2 * self.n_critics if name == "log_alpha" else super()._model_id(name)

    def close(self):
        if getattr(self, "_h", None):
            _lib.check(_lib.lib().bdr_agent_destroy(self._h))   # (refused for a member of a live CandleSacGroup: the group owns it)
            self._h = None

    def update_on_batch(self, obs, act, next_obs, reward, is_terminated, is_truncated, z_pi=None, z_next=None) -> dict:
        """One Sac::opt_ iteration.  z_pi / z_next: [n, act_dim] N(0,1) draws for a and next_a in train mode (None: the agent's
        device stream)."""
        f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
        obs, act, next_obs, reward, z_pi, z_next = map(f, (obs, act, next_obs, reward, z_pi, z_next))
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        trunc = np.ascontiguousarray(is_truncated, dtype=np.int8)
        n, A = len(reward), self.config.act_dim
        for z in (z_pi, z_next):
            if z is not None and z.size != n * A:
                raise ValueError(f"noise rows must hold {n} x {A} values")
        rec = np.zeros(3, np.float32)
        _lib.check(_lib.lib().bdr_candle_sac_update_on_batch(self._h, n, _p(obs), _p(act), _p(next_obs), _p(reward), _p(term),
                                                             _p(trunc), _p(z_pi), _p(z_next), _p(rec)))
        return {k: float(v) for k, v in zip(RECORD_KEYS, rec)}

    PROBES = {"a": 0, "logp": 1, "q_min": 2, "next_a": 3, "next_logp": 4, "tgt": 5, "q_pred": 6, "dq_da": 7}

    def probe(self, what: str, batch: int) -> np.ndarray:
        """Intermediates of the last update (bdr_candle_sac_probe): q_pred [n_critics, B], a / next_a / dq_da [B, act_dim], the
        others [B]."""
        A = self.config.act_dim
        shape = {"q_pred": (self.n_critics, batch), "a": (batch, A), "next_a": (batch, A), "dq_da": (batch, A)}.get(what, (batch,))
        out = np.empty(shape, np.float32)
        _lib.check(_lib.lib().bdr_candle_sac_probe(self._h, self.PROBES[what], _p(out), out.size))
        return out
