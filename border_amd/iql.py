"""Host-side mirror of border-candle-agent's Iql agent over the C ABI (offline RL).

  IqlConfig            border-candle-agent/src/iql/config.rs (defaults :109-125; `.lambda(v)` sets inv_lambda = 1 / v)
  ValueConfig          iql/value.rs (value_config: MlpConfig, opt_config)
  MultiCriticConfig    util/critic.rs:35-43 (n_nets 2, q_config, opt_config, tau 0.005)
  GaussianActorConfig  util/actor.rs:36-55 (policy_config: Mlp3's MlpConfig, opt_config, min/max_log_std, action_limit)
  ActionLimit          util/actor.rs:29-32 (Tanh{action_scale} | Clamp{action_min, action_max})
  CandleMlpConfig      mlp/config.rs:6-11 (activation_out: "None" | "ReLU")
  AgentHandle          what the handles of Iql, Awac (border_amd.awac) and Bc (border_amd.bc) share over the C ABI
  CandleAgent          on it, what Iql and Awac share: actor + critics + targets, the noise stream, the f32 Policy::sample
  Iql                  iql/base.rs (Agent, Policy::sample, SyncModel ships the actor)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .dqn import OptimizerConfig
from .replay import SimpleReplayBuffer

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


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


ROLES = {"param": 0, "grad": 100, "exp_avg": 200, "exp_avg_sq": 300}


class AgentHandle:
    """The handle of an agent on the dense-agent core (csrc/dense_agent.hpp): its lifecycle, Agent::opt, the parameter views,
    SyncModel (the model SYNC_MODEL) and the checkpoint files CKPT_STEMS.  A subclass names its entry points (KIND), its models
    (WHICH, or _model_id) and adds its update_on_batch, probes and Policy::sample."""
    KIND = ""                        # "iql" | "awac" | "bc": the bdr_<KIND>_* entry points
    CKPT_STEMS: Tuple[str, ...] = ()
    SYNC_MODEL = ""                  # the model SyncModel ships (model 0) and the default of the parameter views
    WHICH: dict = {}                 # ParamExchange / ModelMailbox names of model 0

    def __init__(self, config):
        self.config = config
        h = C.c_void_p()
        c = config.to_c()
        _lib.check(getattr(_lib.lib(), f"bdr_{self.KIND}_create")(C.byref(c), C.byref(h)))
        self._h = h

    @classmethod
    def build(cls, config):
        return cls(config)

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().bdr_agent_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _model_id(self, name: str) -> int:
        return self.WHICH[name]

    # model ids (bdr_agent_get_params `which`)
    def which(self, name: Optional[str] = None, role: str = "param") -> int:
        return self._model_id(name or self.SYNC_MODEL) + ROLES[role]

    def arena_device_ptr(self, which: Optional[str] = None):
        ptr, n = C.c_void_p(), C.c_uint64()
        _lib.check(_lib.lib().bdr_agent_arena_device_ptr(self._h, self.WHICH[which or self.SYNC_MODEL], C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def train(self):
        _lib.check(_lib.lib().bdr_agent_set_train(self._h, 1))

    def eval(self):
        _lib.check(_lib.lib().bdr_agent_set_train(self._h, 0))

    def opt(self, buffer: SimpleReplayBuffer) -> None:
        _lib.check(_lib.lib().bdr_agent_opt(self._h, buffer.handle))

    def opt_with_record(self, buffer: SimpleReplayBuffer) -> dict:
        from .dqn import opt_with_named_record
        return opt_with_named_record(self._h, buffer)

    ACT_PATHS = {"default": 0, "layers": 1, "fused": 2}   # BDR_ACT_PATH_*

    def set_act_path(self, path: str) -> None:
        """How Policy::sample runs: "layers" (pack, one launch per layer, the sample kernel), "fused" (k_dense_act: one launch from the
        raw rows to the action; same bits) or "default".  "fused" on a network it does not cover raises BdrError."""
        _lib.check(_lib.lib().bdr_agent_set_act_path(self._h, self.ACT_PATHS[path]))

    def _raw_out(self, n: int):
        """(result array, is it an index array) of a sample of n rows"""
        return np.empty((n, self.config.act_dim), np.float32), False

    def sample_raw(self, rows, obs_norm=None) -> np.ndarray:
        """Policy::sample on raw environment rows (bdr_agent_sample_raw): float32 or float64 host rows [n, obs_dim], rounded to
        float32 and - with `obs_norm`, an ObsNormalizer - normalised on the device with the bits of ObsNormalizer.apply."""
        rows = np.asarray(rows)
        if rows.dtype != np.float32:
            rows = rows.astype(np.float64, copy=False)
        rows = np.ascontiguousarray(rows).reshape(-1, self.config.obs_dim)
        out, disc = self._raw_out(rows.shape[0])
        code = _lib.BDR_DTYPE_F32 if rows.dtype == np.float32 else _lib.BDR_DTYPE_F64
        _lib.check(_lib.lib().bdr_agent_sample_raw(self._h, obs_norm.handle if obs_norm is not None else None, rows.shape[0], _p(rows), code, 0, 0,
                                                   None if disc else _p(out), _p(out) if disc else None))
        return out

    def sample_raw_device(self, ptr: int, n: int, row_stride: int, dtype=np.float32, obs_norm=None) -> np.ndarray:
        """The same for rows in HBM: row k at ptr + k * row_stride bytes, obs_dim elements of `dtype`."""
        out, disc = self._raw_out(n)
        code = _lib.BDR_DTYPE_F32 if np.dtype(dtype) == np.float32 else _lib.BDR_DTYPE_F64
        _lib.check(_lib.lib().bdr_agent_sample_raw(self._h, obs_norm.handle if obs_norm is not None else None, n, C.c_void_p(ptr), code, 1, row_stride,
                                                   None if disc else _p(out), _p(out) if disc else None))
        return out

    def profile_read(self) -> list:
        """[(bracket name, mean milliseconds)] of the launches recorded since profile_enable (bdr_agent_profile_read), in launch order."""
        n = C.c_uint64(256)
        names, ms = C.create_string_buffer(16384), np.zeros(256, np.float32)
        _lib.check(_lib.lib().bdr_agent_profile_read(self._h, names, len(names), _p(ms), C.byref(n)))
        keys = [k for k in names.value.decode().split("\n") if k]
        return [(k, float(ms[i])) for i, k in enumerate(keys[:n.value])]

    def profile_enable(self, on: bool = True):
        _lib.check(_lib.lib().bdr_agent_profile_enable(self._h, int(on)))

    def sync(self):
        _lib.check(_lib.lib().bdr_agent_sync(self._h))

    @property
    def n_opts(self) -> int:
        n = C.c_uint64()
        _lib.check(_lib.lib().bdr_agent_n_opts(self._h, C.byref(n)))
        return n.value

    def param_count(self, name: Optional[str] = None) -> int:
        n = C.c_uint64()
        _lib.check(_lib.lib().bdr_agent_param_count_of(self._h, self.which(name), C.byref(n)))
        return n.value

    def get_params(self, name: Optional[str] = None, role="param") -> np.ndarray:
        out = np.empty(self.param_count(name), np.float32)
        _lib.check(_lib.lib().bdr_agent_get_params(self._h, self.which(name, role), _p(out), out.size))
        return out

    def set_params(self, params, name: Optional[str] = None, role="param") -> None:
        p = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
        _lib.check(_lib.lib().bdr_agent_set_params(self._h, self.which(name, role), _p(p), p.size))

    def model_info(self):
        """SyncModel::model_info: the parameters of SYNC_MODEL."""
        return self.n_opts, self.get_params()

    def sync_model(self, model_info) -> None:
        self.set_params(model_info)

    def set_checkpoint_format(self, fmt: str) -> None:
        """"tch" (default): the reference's `<stem>.pt` files (safetensors, as candle's VarMap writes them); "safetensors":
        `<stem>.safetensors`."""
        from .checkpoint import FORMATS
        _lib.check(_lib.lib().bdr_agent_set_checkpoint_format(self._h, FORMATS[fmt]))
        self._ckpt_ext = {"tch": ".pt", "safetensors": ".safetensors"}[fmt]

    def save_params(self, path: str):
        """The files of CKPT_STEMS (the candle agents' critic.tgt holds the ONLINE critics, util/critic.rs:272-285)."""
        os.makedirs(path, exist_ok=True)
        _lib.check(_lib.lib().bdr_agent_save_params(self._h, path.encode()))
        ext = getattr(self, "_ckpt_ext", ".pt")
        return [os.path.join(path, stem + ext) for stem in self.CKPT_STEMS]

    def load_params(self, path: str):
        _lib.check(_lib.lib().bdr_agent_load_params(self._h, path.encode()))


class CandleAgent(AgentHandle):
    """The handle of a candle-family agent (csrc/candle_actor.hpp): the models of an actor with critics and their targets, the
    device noise stream and the f32 Policy::sample (bdr_<KIND>_sample*); SyncModel ships the actor."""
    SYNC_MODEL = "actor"
    WHICH = {"actor": 0, "pi": 0, "qnet": 0}   # ParamExchange / ModelMailbox: SyncModel ships the actor == model 0

    @property
    def n_critics(self) -> int:
        return self.config.critic_config.n_nets

    def _model_id(self, name: str) -> int:
        """actor 0, critic_i 1 + i, critic_tgt_i 1 + n_critics + i; an agent's own models follow"""
        nc = self.n_critics
        if name.startswith("critic_tgt_"):
            return 1 + nc + int(name[len("critic_tgt_"):])
        if name.startswith("critic_"):
            return 1 + int(name[len("critic_"):])
        return {"actor": 0}[name]

    def draw_noise(self, n: int) -> np.ndarray:
        """n draws of the agent's device noise stream (bdr_agent_draw_noise): the N(0,1) numbers of Policy::sample in train mode."""
        from .dqn import draw_noise
        return draw_noise(self._h, n)

    def sample(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        out = np.empty((obs.shape[0], self.config.act_dim), np.float32)
        _lib.check(getattr(_lib.lib(), f"bdr_{self.KIND}_sample")(self._h, obs.shape[0], _p(obs), _p(out)))
        return out

    def sample_device(self, obs_dev: int, n: int, row_stride: int) -> np.ndarray:
        out = np.empty((n, self.config.act_dim), np.float32)
        _lib.check(getattr(_lib.lib(), f"bdr_{self.KIND}_sample_device")(self._h, n, C.c_void_p(obs_dev), row_stride, _p(out)))
        return out


class Iql(CandleAgent):
    """iql/base.rs; checkpoints (iql/base.rs:292-302): actor, critic, critic.tgt, value."""
    KIND = "iql"
    CKPT_STEMS = ("actor", "critic", "critic.tgt", "value")

    def _model_id(self, name: str) -> int:
        return 1 + 2 * self.n_critics if name == "value" else super()._model_id(name)

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
