"""Host-side mirror of border-candle-agent's Bc agent (behaviour cloning) over the C ABI.

  BcConfig        border-candle-agent/src/bc/config.rs (defaults :66-75: batch_size 1, action_type Discrete, device None,
                  record_verbose_level 0)
  BcModelConfig   bc/model.rs (policy_model_config: the Mlp's MlpConfig, opt_config: OptimizerConfig::default() = AdamW)
  BcActionType    bc/config.rs (Discrete | Continuous)
  Bc              bc/base.rs (Agent, Policy::sample, SyncModel ships the policy; train() / eval() do nothing, is_train() is false)

The policy is a plain Mlp whose activation_out may be any of "None", "ReLU", "Tanh", "Sigmoid" (CandleMlpConfig of border_amd.iql).
kernel_form picks how one update is launched: "default", "general" (three launches for the last layer, any act_dim) or "fused"
(k_bc_head, act_dim <= 64, the last layer's weights staged in LDS; head_rows is its row block, 0: the measured default) or "fused_mfma"
(k_bc_head_mfma, the same launch on the FP32 MFMA, 32 rows per workgroup).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from .dqn import OptimizerConfig
from .handle import DenseHandle
from .iql import ROLES, AgentHandle, CandleMlpConfig, _p  # noqa: F401  (ROLES: importable from here as before)


class BcActionType:
    Discrete = "Discrete"
    Continuous = "Continuous"


ACTION_TYPES = {BcActionType.Discrete: 0, BcActionType.Continuous: 1}   # BDR_BC_ACTION_*
KERNEL_FORMS = {"default": 0, "general": 1, "fused": 2, "fused_mfma": 3}   # BDR_BC_KERNEL_*


@dataclass
class BcModelConfig:
    policy_model_config: CandleMlpConfig = field(default_factory=CandleMlpConfig)
    opt_config: OptimizerConfig = field(default_factory=lambda: OptimizerConfig.AdamW(1e-3))


@dataclass
class BcConfig:
    obs_dim: int = 0
    act_dim: int = 0
    policy_model_config: BcModelConfig = field(default_factory=BcModelConfig)
    batch_size: int = 1
    action_type: str = BcActionType.Discrete
    device: Optional[int] = None
    record_verbose_level: int = 0
    seed: int = 0
    kernel_form: str = "default"
    head_rows: int = 0

    def to_c(self) -> _lib.BcConfigC:
        c = _lib.BcConfigC()
        _lib.lib().bdr_bc_config_default(C.byref(c))
        c.obs_dim, c.act_dim = self.obs_dim, self.act_dim
        self.policy_model_config.policy_model_config.fill(c.policy)
        c.opt.fill(self.policy_model_config.opt_config)
        c.lr = self.policy_model_config.opt_config.lr
        c.batch_size, c.action_type = self.batch_size, ACTION_TYPES[self.action_type]
        c.device = -1 if self.device is None else self.device
        c.record_verbose_level, c.seed = self.record_verbose_level, self.seed
        c.kernel_form, c.head_rows = KERNEL_FORMS[self.kernel_form], self.head_rows
        return c


class Bc(DenseHandle):
    """bc/base.rs; checkpoint (bc/base.rs:138-153): policy_model.pt, or policy_model.safetensors (set_checkpoint_format).
    train() / eval() switch nothing (bc/base.rs:104-106)."""
    KIND = "bc"
    CKPT_STEMS = ("policy_model",)
    SYNC_MODEL = "policy"
    WHICH = {"policy": 0, "actor": 0, "pi": 0, "qnet": 0}   # ParamExchange / ModelMailbox: SyncModel ships the policy == model 0
    PROBES = {"pred": 0, "dz": 1}

    def close(self):
        if getattr(self, "_h", None):
            _lib.check(_lib.lib().bdr_agent_destroy(self._h))   # (refused for a member of a live BcGroup: the group owns it)
            self._h = None

    def update_on_batch(self, obs, act) -> dict:
        """One Bc::opt_ (bc/base.rs:167-198) on host rows; the record's one key is "loss"."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        act = np.ascontiguousarray(act, dtype=np.float32)
        n = obs.shape[0]
        if obs.size != n * self.config.obs_dim or act.size != n * self.config.act_dim:
            raise ValueError(f"rows must hold {n} x {self.config.obs_dim} observations and {n} x {self.config.act_dim} actions")
        rec = np.zeros(1, np.float32)
        _lib.check(_lib.lib().bdr_bc_update_on_batch(self._h, n, _p(obs), _p(act), _p(rec)))
        return {"loss": float(rec[0])}

    def probe(self, what: str, batch: int) -> np.ndarray:
        """Intermediates of the last update (bdr_bc_probe): pred, dz [B, act_dim]."""
        out = np.empty((batch, self.config.act_dim), np.float32)
        _lib.check(_lib.lib().bdr_bc_probe(self._h, self.PROBES[what], _p(out), out.size))
        return out

    def _out(self, n: int):
        if self.config.action_type == BcActionType.Discrete:
            return np.empty(n, np.int64), True
        return np.empty((n, self.config.act_dim), np.float32), False

    _raw_out = _out   # DenseHandle.sample_raw / sample_raw_device: Discrete agents return indices

    def sample(self, obs) -> np.ndarray:
        """Policy::sample (bc/base.rs:49-59): [n, act_dim] f32 (Continuous) or [n] i64 argmax indices (Discrete)"""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        out, disc = self._out(obs.shape[0])
        _lib.check(_lib.lib().bdr_bc_sample(self._h, obs.shape[0], _p(obs), None if disc else _p(out), _p(out) if disc else None))
        return out

    def sample_device(self, obs_dev: int, n: int, row_stride: int) -> np.ndarray:
        out, disc = self._out(n)
        _lib.check(_lib.lib().bdr_bc_sample_device(self._h, n, C.c_void_p(obs_dev), row_stride, None if disc else _p(out),
                                                   _p(out) if disc else None))
        return out
