"""Host-side mirror of border-tch-agent's Iqn agent over the C ABI.

  IqnConfig       border-tch-agent/src/iqn/config.rs (defaults :50-67)
  IqnModelConfig  border-tch-agent/src/iqn/model/config.rs (feature_dim, embed_dim, opt_config)
  IqnSample       border-tch-agent/src/iqn/model/base.rs:327-387
  Iqn             border-tch-agent/src/iqn/base.rs
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .dqn import AtariCnnConfig, MlpConfig, OptimizerConfig, TchValueAgent
from .handle import _p

IQN_SAMPLE = {"Const10": 0, "Const32": 1, "Uniform10": 2, "Uniform8": 3, "Uniform32": 4, "Uniform64": 5, "Median": 6}


@dataclass
class IqnConfig:
    f_config: object = field(default_factory=lambda: AtariCnnConfig(n_stack=4, out_dim=0, skip_linear=True))
    feature_dim: int = 3136
    embed_dim: int = 64
    m_units: Tuple[int, ...] = (512,)            # merge net M = Mlp(feature_dim, units, n_actions)
    n_actions: int = 0
    lr: float = 1e-4
    opt_config: Optional[OptimizerConfig] = None   # IqnModelConfig.opt_config (iqn/model/config.rs:50); None = OptimizerConfig.Adam(lr)
    soft_update_interval: int = 1
    n_updates_per_opt: int = 1
    batch_size: int = 1
    discount_factor: float = 0.99
    tau: float = 0.005
    sample_percents_pred: str = "Uniform8"
    sample_percents_tgt: str = "Uniform8"
    sample_percents_act: str = "Const32"
    train: bool = False
    device: Optional[int] = None
    seed: int = 0
    arithmetic: str = "bf16x3_6"                 # BDR_ARITH_* (not a reference field): "bf16x3_6" | "f32_exact"

    def to_c(self) -> _lib.IqnConfigC:
        c = _lib.IqnConfigC()
        _lib.lib().bdr_iqn_config_default(C.byref(c))
        q = self.f_config
        if isinstance(q, AtariCnnConfig):
            c.psi.kind, c.psi.n_stack = 0, q.n_stack
        else:
            c.psi.kind, c.psi.in_dim, c.psi.n_units, c.psi.out_dim = 1, q.in_dim, len(q.units), q.out_dim
            for i, u in enumerate(q.units):
                c.psi.units[i] = u
            c.psi.activation_out = int(q.activation_out)
        c.feature_dim, c.embed_dim, c.n_f_units, c.n_actions, c.lr = self.feature_dim, self.embed_dim, len(self.m_units), self.n_actions, self.lr
        for i, u in enumerate(self.m_units):
            c.f_units[i] = u
        c.soft_update_interval, c.n_updates_per_opt, c.batch_size = self.soft_update_interval, self.n_updates_per_opt, self.batch_size
        c.discount_factor, c.tau = self.discount_factor, self.tau
        c.sample_percents_pred, c.sample_percents_tgt, c.sample_percents_act = (IQN_SAMPLE[self.sample_percents_pred],
                                                                               IQN_SAMPLE[self.sample_percents_tgt],
                                                                               IQN_SAMPLE[self.sample_percents_act])
        c.train, c.device, c.seed = int(self.train), -1 if self.device is None else self.device, self.seed
        if self.opt_config is not None:
            c.lr = self.opt_config.lr
            c.opt.fill(self.opt_config)
        c.arithmetic = _lib.ARITHMETIC[self.arithmetic]
        return c


class Iqn(TchValueAgent):
    """iqn/base.rs; checkpoints iqn, iqn_tgt; the models are named as the tch Dqn names them ("qnet" is "iqn")."""
    KIND = "iqn"
    CKPT_STEMS = ("iqn", "iqn_tgt")
    SYNC_MODEL = "iqn"
    WHICH = {"qnet": 0, "iqn": 0, "iqn_tgt": 1, "exp_avg": 2, "exp_avg_sq": 3, "grad": 4, "max_exp_avg_sq": 5}

    def __init__(self, config: IqnConfig):
        super().__init__(config)
        self.n_actions = config.n_actions

    # the parameter views under this class's own signatures: `iqn` is the literal default
    def arena_device_ptr(self, which="iqn"):
        return super().arena_device_ptr(which)

    def get_params(self, which="iqn") -> np.ndarray:
        return super().get_params(which)

    def set_params(self, params, which="iqn") -> None:
        super().set_params(params, which)

    def update_on_batch(self, obs, act, next_obs, reward, is_terminated, tau_pred, tau_tgt) -> dict:
        reward = np.ascontiguousarray(reward, dtype=np.float32)
        n = len(reward)
        obs, next_obs = np.ascontiguousarray(obs), np.ascontiguousarray(next_obs)
        act = np.ascontiguousarray(act, dtype=np.int64).reshape(n)
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        tp, tt = np.ascontiguousarray(tau_pred, dtype=np.float32), np.ascontiguousarray(tau_tgt, dtype=np.float32)
        loss = np.zeros(1, np.float32)
        _lib.check(_lib.lib().bdr_iqn_update_on_batch(self._h, n, _p(obs), _p(act), _p(next_obs), _p(reward), _p(term),
                                                      _p(tp), tp.shape[1], _p(tt), tt.shape[1], _p(loss)))
        return dict(loss_critic=float(loss[0]))

    def forward(self, obs, tau, which="iqn") -> np.ndarray:
        obs, tau = np.ascontiguousarray(obs), np.ascontiguousarray(tau, dtype=np.float32)
        n, nt = tau.shape
        z = np.empty((n, nt, self.config.n_actions), np.float32)
        _lib.check(_lib.lib().bdr_iqn_forward(self._h, self.WHICH[which], n, _p(obs), _p(tau), nt, _p(z)))
        return z

    PROBE = {"cos": 0, "phi": 1, "psi": 2, "dlin": 3, "dpsi": 4, "tgt": 5, "loss_row": 6, "a1": 7, "a2": 8, "dy2": 9, "dy1": 10,
             "f_act": 16, "f_dy": 32, "psi_act": 48, "psi_dy": 64}   # BDR_IQN_PROBE_*

    def probe(self, what: str, rows: int, i: int = 0, cols: Optional[int] = None) -> np.ndarray:
        """bdr_iqn_probe: the raw buffer [rows][ld] that the last forward / update left behind, padding columns included (they must be
        exactly 0, and a test can assert it).  rows: B * N for cos, phi, dlin, f_act, f_dy; B for the others.  i: the layer of f_act /
        f_dy (merge net, the last one is z / dz) and psi_act / psi_dy (Mlp feature extractor).  cols: tgt's n_tgt.  A wrong row count
        is an error of the library, never a short or long read.  forward() and qvalues() overwrite (or reallocate) these buffers."""
        c, pad = self.config, lambda x: (x + 63) // 64 * 64
        cnn = isinstance(c.f_config, AtariCnnConfig)
        f_ld = [pad(u) for u in tuple(c.m_units) + (c.n_actions,)]
        psi_ld = [] if cnn else [pad(u) for u in tuple(c.f_config.units) + (c.f_config.out_dim,)]
        ldf = 3136 if cnn else pad(c.feature_dim)
        ld = {"cos": pad(c.embed_dim), "phi": pad(c.feature_dim), "dlin": pad(c.feature_dim), "psi": ldf, "dpsi": ldf, "tgt": cols, "loss_row": 1,
              "a1": 400 * 32, "dy1": 400 * 32, "a2": 81 * 64, "dy2": 81 * 64}.get(what)
        if what in ("f_act", "f_dy"):
            ld = f_ld[i]
        elif what in ("psi_act", "psi_dy"):
            ld = psi_ld[i]
        if ld is None:
            raise ValueError("unknown probe %r (or tgt without cols)" % (what,))
        out = np.empty((rows, ld), np.float32)
        _lib.check(_lib.lib().bdr_iqn_probe(self._h, self.PROBE[what] + (i if self.PROBE[what] >= 16 else 0), _p(out), out.size))
        return out

    def qvalues(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs)
        q = np.empty((obs.shape[0], self.config.n_actions), np.float32)
        _lib.check(_lib.lib().bdr_iqn_qvalues(self._h, obs.shape[0], _p(obs), _p(q), None))
        return q
