"""What every agent handle shares over the C ABI.

  AgentHandle   the lifecycle, Agent::opt, `which`, the parameter views, SyncModel, the checkpoint format and file names, profiling
  DenseHandle   on it, set_act_path and sample_raw: the agents of the dense-agent core
  CandleAgent   on that, what the candle-family agents share: actor + critics + targets, the noise stream, the f32 Policy::sample
  ROLES         the `which` offsets of a model's gradient and optimizer state
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .replay import SimpleReplayBuffer


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def record_keys(handle) -> list:
    names = C.create_string_buffer(8192)
    n = C.c_int32()
    _lib.check(_lib.lib().bdr_agent_record_keys(handle, names, 8192, C.byref(n)))
    return names.value.decode().split("\n")[:n.value]


def opt_with_named_record(handle, buffer) -> dict:
    """bdr_agent_opt_with_scalars + bdr_agent_record_keys: the reference's Record of one opt_with_record call."""
    out = np.zeros(128, np.float32)
    n = C.c_int32()
    _lib.check(_lib.lib().bdr_agent_opt_with_scalars(handle, buffer.handle, _p(out), 128, C.byref(n)))
    return {k: float(v) for k, v in zip(record_keys(handle), out[:n.value])}


def draw_noise(handle, n: int) -> np.ndarray:
    out = np.empty(n, np.float32)
    _lib.check(_lib.lib().bdr_agent_draw_noise(handle, n, _p(out)))
    return out


ROLES = {"param": 0, "grad": 100, "exp_avg": 200, "exp_avg_sq": 300}


class AgentHandle:
    """The handle of an agent: its lifecycle, Agent::opt, the parameter views (the library's model table, csrc/param_table.hpp),
    SyncModel (the model SYNC_MODEL) and the checkpoint files CKPT_STEMS.  A subclass names its entry points (KIND), its models
    (WHICH, or _model_id), its roles and file extensions where they differ, and adds its update_on_batch, probes and Policy::sample."""
    KIND = ""                        # "dqn" | "iql" | "bc" ...: the bdr_<KIND>_* entry points
    CKPT_STEMS: Tuple[str, ...] = ()
    CKPT_EXTS = {"tch": ".pt", "safetensors": ".safetensors"}   # the candle agents' names; the tch agents write <stem>.pt.tch
    ROLES = ROLES
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
        return self._model_id(name or self.SYNC_MODEL) + self.ROLES[role]

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
        return opt_with_named_record(self._h, buffer)

    def is_train(self) -> bool:
        v = C.c_int32()
        _lib.check(_lib.lib().bdr_agent_is_train(self._h, C.byref(v)))
        return bool(v.value)

    def draw_noise(self, n: int) -> np.ndarray:
        """n draws of the agent's device noise stream (bdr_agent_draw_noise)."""
        return draw_noise(self._h, n)

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
        """"tch" (default): the reference's files - `<stem>.pt.tch` libtorch archives of the tch agents, `<stem>.pt` of the candle
        agents (safetensors, as candle's VarMap writes them); "safetensors": `<stem>.safetensors`."""
        from .checkpoint import FORMATS
        _lib.check(_lib.lib().bdr_agent_set_checkpoint_format(self._h, FORMATS[fmt]))
        self._ckpt_ext = self.CKPT_EXTS[fmt]

    def save_params(self, path: str):
        """The files of CKPT_STEMS (the candle agents' critic.tgt holds the ONLINE critics, util/critic.rs:272-285)."""
        os.makedirs(path, exist_ok=True)
        _lib.check(_lib.lib().bdr_agent_save_params(self._h, path.encode()))
        ext = getattr(self, "_ckpt_ext", self.CKPT_EXTS["tch"])
        return [os.path.join(path, stem + ext) for stem in self.CKPT_STEMS]

    def load_params(self, path: str):
        _lib.check(_lib.lib().bdr_agent_load_params(self._h, path.encode()))


class DenseHandle(AgentHandle):
    """On AgentHandle, what the library serves for the agents of the dense-agent core (IQL, AWAC, BC, the candle SAC and DQN): the
    acting path and Policy::sample on raw rows; their configs carry obs_dim and act_dim."""
    ACT_PATHS = {"default": 0, "layers": 1, "fused": 2}   # BDR_ACT_PATH_*

    def set_act_path(self, path: str) -> None:
        """How Policy::sample runs: "layers" (pack, one launch per layer, the sample kernel), "fused" (k_dense_act: one launch from the
        raw rows to the action; same bits) or "default".  "fused" on a network it does not cover raises BdrError."""
        _lib.check(_lib.lib().bdr_agent_set_act_path(self._h, self.ACT_PATHS[path]))

    def get_hyper(self, name) -> float:
        """One settable hyperparameter (bdr_agent_hyper_get): a name of _lib.HYPER_IDS - "lr" and "beta1" ... of BC; "lr_actor",
        "lr_critic", "lr_value", "actor_beta1" ..., "gamma", "critic_tau", "tau_iql", "inv_lambda", "exp_adv_max", "ent_coef_lr",
        "target_entropy" of the others - or its BDR_HYPER_* id.  A name the agent's kind does not have raises BdrError."""
        return _lib.agent_get_hyper(self._h, name)

    def set_hyper(self, name, value: float) -> None:
        """Set it (bdr_agent_hyper_set): in force from the agent's next update, standalone or as a group member.  A value outside
        the field's range raises BdrError.  (`config` keeps what the agent was built with.)"""
        _lib.agent_set_hyper(self._h, name, value)

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


class CandleAgent(DenseHandle):
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

    def sample(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        out = np.empty((obs.shape[0], self.config.act_dim), np.float32)
        _lib.check(getattr(_lib.lib(), f"bdr_{self.KIND}_sample")(self._h, obs.shape[0], _p(obs), _p(out)))
        return out

    def sample_device(self, obs_dev: int, n: int, row_stride: int) -> np.ndarray:
        out = np.empty((n, self.config.act_dim), np.float32)
        _lib.check(getattr(_lib.lib(), f"bdr_{self.KIND}_sample_device")(self._h, n, C.c_void_p(obs_dev), row_stride, _p(out)))
        return out
