"""Host-side mirror of border-candle-agent's Iql agent over the C ABI (offline RL).

  IqlConfig            border-candle-agent/src/iql/config.rs (defaults :109-125; `.lambda(v)` sets inv_lambda = 1 / v)
  ValueConfig          iql/value.rs (value_config: MlpConfig, opt_config)
  MultiCriticConfig    util/critic.rs:35-43 (n_nets 2, q_config, opt_config, tau 0.005)
  GaussianActorConfig  util/actor.rs:36-55 (policy_config: Mlp3's MlpConfig, opt_config, min/max_log_std, action_limit)
  ActionLimit          util/actor.rs:29-32 (Tanh{action_scale} | Clamp{action_min, action_max})
  CandleMlpConfig      mlp/config.rs:6-11 (activation_out: "None" | "ReLU")
  AgentHandle, CandleAgent   border_amd.handle (re-exported here)
  Iql                  iql/base.rs (Agent, Policy::sample, SyncModel ships the actor)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .dqn import OptimizerConfig
from .handle import ROLES, AgentHandle, CandleAgent, _p  # noqa: F401  (their home is border_amd.handle; importable from here as before)

ACTIVATIONS = {"None": 0, "ReLU": 1, "Tanh": 2, "Sigmoid": 3}   # lib.rs:58-63 (Tanh / Sigmoid: BC only; IQL and AWAC reject them)


@dataclass
class CandleMlpConfig:
    units: Tuple[int, ...] = (256, 256)
    activation_out: str = "None"

    def fill(self, m: "_lib.MlpConfigC") -> None:
        m.n_units = len(self.units)
        for i, u in enumerate(self.units):
            m.units[i] = u
        m.activation_out = ACTIVATIONS[self.activation_out]


@dataclass
class ActionLimit:
    kind: str = "Clamp"          # "Clamp" | "Tanh"
    action_min: float = -1.0
    action_max: float = 1.0
    action_scale: float = 1.0

    @classmethod
    def Clamp(cls, action_min: float = -1.0, action_max: float = 1.0) -> "ActionLimit":
        return cls("Clamp", action_min, action_max)

    @classmethod
    def Tanh(cls, action_scale: float = 1.0) -> "ActionLimit":
        return cls("Tanh", action_scale=action_scale)


@dataclass
class ValueConfig:
    value_config: CandleMlpConfig = field(default_factory=CandleMlpConfig)
    opt_config: OptimizerConfig = field(default_factory=lambda: OptimizerConfig.Adam(3e-4))


@dataclass
class MultiCriticConfig:
    n_nets: int = 2
    q_config: CandleMlpConfig = field(default_factory=CandleMlpConfig)
    opt_config: OptimizerConfig = field(default_factory=lambda: OptimizerConfig.Adam(3e-4))
    tau: float = 0.005


@dataclass
class GaussianActorConfig:
    policy_config: CandleMlpConfig = field(default_factory=CandleMlpConfig)
    opt_config: OptimizerConfig = field(default_factory=lambda: OptimizerConfig.Adam(3e-4))
    min_log_std: float = -20.0
    max_log_std: float = 2.0
    action_limit: ActionLimit = field(default_factory=ActionLimit.Clamp)
    kind: str = "Mlp3"   # "Mlp3" | "Mlp2" (mlp/mlp2.rs): read by CandleSacConfig only; IQL and AWAC build Mlp3


@dataclass
class IqlConfig:
    obs_dim: int = 0
    act_dim: int = 0
    value_config: ValueConfig = field(default_factory=ValueConfig)
    critic_config: MultiCriticConfig = field(default_factory=MultiCriticConfig)
    actor_config: GaussianActorConfig = field(default_factory=GaussianActorConfig)
    gamma: float = 0.99
    tau_iql: float = 0.7
    inv_lambda: float = 10.0
    n_updates_per_opt: int = 1
    batch_size: int = 1
    adv_softmax: bool = False
    critic_loss: str = "Mse"
    exp_adv_max: float = 100.0
    train: bool = False
    seed: int = 0
    device: Optional[int] = None

    def lambda_(self, v: float) -> "IqlConfig":
        """IqlConfig::lambda (iql/config.rs): inv_lambda = 1 / v"""
        self.inv_lambda = 1.0 / v
        return self

    def to_c(self) -> _lib.IqlConfigC:
        c = _lib.IqlConfigC()
        _lib.lib().bdr_iql_config_default(C.byref(c))
        c.obs_dim, c.act_dim = self.obs_dim, self.act_dim
        self.value_config.value_config.fill(c.value)
        self.actor_config.policy_config.fill(c.actor)
        self.critic_config.q_config.fill(c.critic)
        c.n_critics, c.critic_tau = self.critic_config.n_nets, self.critic_config.tau
        for name, o in (("value", self.value_config.opt_config), ("actor", self.actor_config.opt_config), ("critic", self.critic_config.opt_config)):
            setattr(c, "lr_" + name, o.lr)
            getattr(c, "opt_" + name).fill(o)
        ac = self.actor_config
        c.min_log_std, c.max_log_std = ac.min_log_std, ac.max_log_std
        lim = ac.action_limit
        c.action_limit = {"Clamp": 0, "Tanh": 1}[lim.kind]
        c.action_min, c.action_max, c.action_scale = lim.action_min, lim.action_max, lim.action_scale
        c.gamma, c.tau_iql, c.inv_lambda, c.exp_adv_max = self.gamma, self.tau_iql, self.inv_lambda, self.exp_adv_max
        c.adv_softmax = int(self.adv_softmax)
        c.critic_loss = {"Mse": 0, "SmoothL1": 1}[self.critic_loss]
        c.n_updates_per_opt, c.batch_size, c.train, c.seed = self.n_updates_per_opt, self.batch_size, int(self.train), self.seed
        c.device = -1 if self.device is None else self.device
        return c


class Iql(CandleAgent):
    """iql/base.rs; checkpoints (iql/base.rs:292-302): actor, critic, critic.tgt, value."""
    KIND = "iql"
    CKPT_STEMS = ("actor", "critic", "critic.tgt", "value")

    def _model_id(self, name: str) -> int:
        return 1 + 2 * self.n_critics if name == "value" else super()._model_id(name)

    def close(self):
        if getattr(self, "_h", None):
            _lib.check(_lib.lib().bdr_agent_destroy(self._h))   # (refused for a member of a live IqlGroup: the group owns it)
            self._h = None

    def update_on_batch(self, obs, act, next_obs, reward, is_terminated, is_truncated) -> dict:
        f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        obs, act, next_obs, reward = map(f, (obs, act, next_obs, reward))
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        trunc = np.ascontiguousarray(is_truncated, dtype=np.int8)
        rec = np.zeros(3, np.float32)
        _lib.check(_lib.lib().bdr_iql_update_on_batch(self._h, len(reward), _p(obs), _p(act), _p(next_obs), _p(reward), _p(term),
                                                      _p(trunc), _p(rec)))
        return dict(loss_value=float(rec[0]), loss_critic=float(rec[1]), loss_actor=float(rec[2]))

    PROBES = {"q_tgt_min_value": 0, "v": 1, "u": 2, "tgt": 3, "q_pred": 4, "q_tgt_min_actor": 5, "w": 6, "logp": 7, "v_next": 8, "v_obs": 9}

    def probe(self, what: str, batch: int) -> np.ndarray:
        """Intermediates of the last update (bdr_iql_probe): q_pred [n_critics, B], every other one [B]."""
        shape = (self.n_critics, batch) if what == "q_pred" else (batch,)
        out = np.empty(shape, np.float32)
        _lib.check(_lib.lib().bdr_iql_probe(self._h, self.PROBES[what], _p(out), out.size))
        return out
