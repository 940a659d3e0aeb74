"""Host-side mirror of border-candle-agent's Awac agent over the C ABI (offline and online RL).

  AwacConfig   border-candle-agent/src/awac/config.rs (defaults :120-141; `.lambda_(v)` sets inv_lambda = 1 / v).  The reference's
               tau, min_lstd, max_lstd, reward_scale, n_critics and seed fields are not read by its agent and are not here: the
               soft-update rate is critic_config.tau, the critic count critic_config.n_nets, the log-std bounds actor_config's.
  Awac         awac/base.rs (Agent, Policy::sample, SyncModel ships the actor)

The model configs are IQL's: CandleMlpConfig, ActionLimit, GaussianActorConfig and MultiCriticConfig of border_amd.iql, and so is
CandleAgent, what the two agents' handles share.
batch_size must be >= 2 (include/border_amd.h says why the reference cannot run a one-row batch).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from .iql import CandleAgent, GaussianActorConfig, MultiCriticConfig, _p

RECORD_KEYS = ("loss_critic", "loss_actor", "q_tgt_abs_mean", "adv_mean", "adv_abs_mean", "logp_mean", "reward_mean", "next_q_mean")


@dataclass
class AwacConfig:
    obs_dim: int = 0
    act_dim: int = 0
    actor_config: GaussianActorConfig = field(default_factory=GaussianActorConfig)
    critic_config: MultiCriticConfig = field(default_factory=MultiCriticConfig)
    gamma: float = 0.99
    inv_lambda: float = 10.0
    n_updates_per_opt: int = 1
    batch_size: int = 1
    critic_loss: str = "Mse"
    exp_adv_max: float = 100.0
    adv_softmax: bool = False
    train: bool = False
    seed: int = 0
    device: Optional[int] = None

    def lambda_(self, v: float) -> "AwacConfig":
        """AwacConfig::lambda (awac/config.rs): inv_lambda = 1 / v"""
        self.inv_lambda = 1.0 / v
        return self

    def to_c(self) -> _lib.AwacConfigC:
        c = _lib.AwacConfigC()
        _lib.lib().bdr_awac_config_default(C.byref(c))
        c.obs_dim, c.act_dim = self.obs_dim, self.act_dim
        self.actor_config.policy_config.fill(c.actor)
        self.critic_config.q_config.fill(c.critic)
        c.n_critics, c.critic_tau = self.critic_config.n_nets, self.critic_config.tau
        for name, o in (("actor", self.actor_config.opt_config), ("critic", self.critic_config.opt_config)):
            setattr(c, "lr_" + name, o.lr)
            getattr(c, "opt_" + name).fill(o)
        ac = self.actor_config
        c.min_log_std, c.max_log_std = ac.min_log_std, ac.max_log_std
        lim = ac.action_limit
        c.action_limit = {"Clamp": 0, "Tanh": 1}[lim.kind]
        c.action_min, c.action_max, c.action_scale = lim.action_min, lim.action_max, lim.action_scale
        c.gamma, c.inv_lambda, c.exp_adv_max = self.gamma, self.inv_lambda, self.exp_adv_max
        c.adv_softmax = int(self.adv_softmax)
        c.critic_loss = {"Mse": 0, "SmoothL1": 1}[self.critic_loss]
        c.n_updates_per_opt, c.batch_size, c.train, c.seed = self.n_updates_per_opt, self.batch_size, int(self.train), self.seed
        c.device = -1 if self.device is None else self.device
        return c


class Awac(CandleAgent):
    """awac/base.rs; checkpoints (awac/base.rs:311-320): actor, critic, critic.tgt."""
    KIND = "awac"
    CKPT_STEMS = ("actor", "critic", "critic.tgt")

    def close(self):
        if getattr(self, "_h", None):
            _lib.check(_lib.lib().bdr_agent_destroy(self._h))   # (refused for a member of a live AwacGroup: the group owns it)
            self._h = None

    def update_on_batch(self, obs, act, next_obs, reward, is_terminated, is_truncated, z_pi=None, z_next=None) -> dict:
        """One Awac::opt_ iteration.  z_pi / z_next: [n, act_dim] N(0,1) draws for act_ and next_act in train mode (None: the
        agent's device stream)."""
        f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
        obs, act, next_obs, reward, z_pi, z_next = map(f, (obs, act, next_obs, reward, z_pi, z_next))
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        trunc = np.ascontiguousarray(is_truncated, dtype=np.int8)
        n, A = len(reward), self.config.act_dim
        for z in (z_pi, z_next):
            if z is not None and z.size != n * A:
                raise ValueError(f"noise rows must hold {n} x {A} values")
        rec = np.zeros(8, np.float32)
        _lib.check(_lib.lib().bdr_awac_update_on_batch(self._h, n, _p(obs), _p(act), _p(next_obs), _p(reward), _p(term),
                                                       _p(trunc), _p(z_pi), _p(z_next), _p(rec)))
        return {k: float(v) for k, v in zip(RECORD_KEYS, rec)}

    PROBES = {"q_data_min": 0, "q_pi_min": 1, "adv": 2, "w": 3, "logp": 4, "act_": 5, "next_act": 6, "next_q": 7, "tgt": 8, "q_pred": 9}

    def probe(self, what: str, batch: int) -> np.ndarray:
        """Intermediates of the last update (bdr_awac_probe): q_pred [n_critics, B], act_ / next_act [B, act_dim], the others [B]."""
        shape = {"q_pred": (self.n_critics, batch), "act_": (batch, self.config.act_dim), "next_act": (batch, self.config.act_dim)}.get(what, (batch,))
        out = np.empty(shape, np.float32)
        _lib.check(_lib.lib().bdr_awac_probe(self._h, self.PROBES[what], _p(out), out.size))
        return out
