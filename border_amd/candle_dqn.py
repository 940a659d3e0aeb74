"""Host-side mirror of border-candle-agent's Dqn agent (Mlp or AtariCnn Q-network) over the C ABI.  Not border_amd.Dqn, the tch agent.

  CandleDqnConfig       border-candle-agent/src/dqn/config.rs (defaults :75-102: soft_update_interval 1, n_updates_per_opt 1,
                        batch_size 1, discount_factor 0.99, tau 0.005, train false, explorer Softmax, double_dqn false, critic_loss Mse,
                        record_verbose_level 0).  clip_reward and clip_td_err are carried and read by nothing, as in the reference.
  CandleDqnModelConfig  dqn/model.rs (q_config: the Mlp's MlpConfig, opt_config: OptimizerConfig::default() = AdamW)
                        q_config = AtariCnnConfig(n_stack, out_dim) (atari_cnn/config.rs) builds the AtariCnn form instead: u8 rows of
                        84 * 84 * n_stack bytes, variables c1.weight ... l2.bias; CandleDqnConfig(q_config=AtariCnnConfig(...)) is the
                        short spelling.  `arithmetic` must stay "f32_exact" for it.
  Softmax, EpsilonGreedy  dqn/explorer.rs (the classes of border_amd.dqn); explorer_seed is the seed of the agent's SmallRng, 42 in
                        the reference (dqn/base.rs:274)
  CandleDqn             dqn/base.rs (Agent, Policy::sample -> int64 action indices)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Tuple, Union

import numpy as np

from . import _lib
from .dqn import AtariCnnConfig, EpsilonGreedy, OptimizerConfig, Softmax
from .handle import DenseHandle
from .iql import AgentHandle, CandleMlpConfig, _p  # noqa: F401  (AgentHandle: importable from here as before)


@dataclass
class CandleDqnModelConfig:
    q_config: Union[CandleMlpConfig, AtariCnnConfig] = field(default_factory=CandleMlpConfig)
    opt_config: OptimizerConfig = field(default_factory=lambda: OptimizerConfig.AdamW(1e-3))


@dataclass
class CandleDqnConfig:
    obs_dim: int = 0
    n_actions: int = 0
    model_config: CandleDqnModelConfig = field(default_factory=CandleDqnModelConfig)
    soft_update_interval: int = 1
    n_updates_per_opt: int = 1
    batch_size: int = 1
    discount_factor: float = 0.99
    tau: float = 0.005
    train: bool = False
    explorer: Union[Softmax, EpsilonGreedy] = field(default_factory=Softmax)
    explorer_seed: int = 42
    clip_reward: Optional[float] = None                   # carried, unused (dqn/base.rs:40)
    double_dqn: bool = False
    clip_td_err: Optional[Tuple[float, float]] = None     # carried, unused (dqn/base.rs:138-152 is commented out)
    device: Optional[int] = None
    critic_loss: str = "Mse"
    record_verbose_level: int = 0
    ckpt_format: str = "tch"                              # "tch": qnet.pt / qnet_tgt.pt; "safetensors": *.safetensors
    seed: int = 0
    q_config: Optional[AtariCnnConfig] = None             # the AtariCnn form: replaces model_config.q_config
    arithmetic: str = "f32_exact"                         # AtariCnn form only; "bf16x3_6" is refused by the library

    def __post_init__(self):
        if self.q_config is not None:
            self.model_config = CandleDqnModelConfig(self.q_config, self.model_config.opt_config)
        if self.cnn:
            q = self.model_config.q_config
            self.n_actions = self.n_actions or q.out_dim
            self.obs_dim = 84 * 84 * q.n_stack            # bytes of one u8 row

    @property
    def cnn(self) -> bool:
        return isinstance(self.model_config.q_config, AtariCnnConfig)

    @property
    def act_dim(self) -> int:
        """One int64 action index per row (the width DenseHandle's raw-row helpers ask for)."""
        return 1

    def to_c(self):
        from .checkpoint import FORMATS
        if self.cnn:
            q = self.model_config.q_config
            c = _lib.CandleDqnCnnConfigC()
            _lib.lib().bdr_candle_dqn_cnn_config_default(C.byref(c))
            c.n_stack, c.out_dim, c.skip_linear = q.n_stack, self.n_actions, int(q.skip_linear)
            c.arithmetic = _lib.ARITHMETIC[self.arithmetic]
        else:
            c = _lib.CandleDqnConfigC()
            _lib.lib().bdr_candle_dqn_config_default(C.byref(c))
            c.obs_dim, c.n_actions = self.obs_dim, self.n_actions
            self.model_config.q_config.fill(c.qnet)
        c.opt.fill(self.model_config.opt_config)
        c.lr = self.model_config.opt_config.lr
        c.soft_update_interval, c.n_updates_per_opt, c.batch_size = self.soft_update_interval, self.n_updates_per_opt, self.batch_size
        c.discount_factor, c.tau, c.train, c.double_dqn = self.discount_factor, self.tau, int(self.train), int(self.double_dqn)
        e = self.explorer.to_c(self.explorer_seed)
        for name, _ in e._fields_:
            setattr(c.explorer, name, getattr(e, name))
        if self.clip_reward is not None:
            c.has_clip_reward, c.clip_reward = 1, self.clip_reward
        if self.clip_td_err is not None:
            c.has_clip_td_err, (c.clip_td_err_min, c.clip_td_err_max) = 1, self.clip_td_err
        c.critic_loss = {"Mse": 0, "SmoothL1": 1}[self.critic_loss]
        c.record_verbose_level = self.record_verbose_level
        c.device = -1 if self.device is None else self.device
        c.ckpt_format, c.seed = FORMATS[self.ckpt_format], self.seed
        return c


def _info(info) -> dict:
    return {"eps": info.eps, "is_random": bool(info.is_random), "n_samples_act": info.n_samples_act, "n_samples_best_act": info.n_samples_best_act}


class CandleDqn(DenseHandle):
    """dqn/base.rs; checkpoints (dqn/base.rs:337-351): qnet.pt, qnet_tgt.pt, or *.safetensors (set_checkpoint_format)."""
    KIND = "candle_dqn"
    CKPT_STEMS = ("qnet", "qnet_tgt")
    SYNC_MODEL = "qnet"
    # bdr_agent_get_params `which`: the tch Dqn's numbers
    WHICH = {"qnet": 0, "qnet_tgt": 1, "exp_avg": 2, "exp_avg_sq": 3, "grad": 4}
    PROBES = {"pred": 0, "q_next": 1, "y": 2, "tgt": 3, "dpred": 4}

    def __init__(self, config: CandleDqnConfig):
        self.cnn = config.cnn
        if self.cnn:                                      # bdr_candle_dqn_cnn_create; every other entry point serves both forms
            self.config = config
            h = C.c_void_p()
            c = config.to_c()
            _lib.check(_lib.lib().bdr_candle_dqn_cnn_create(C.byref(c), C.byref(h)))
            self._h = h
        else:
            super().__init__(config)
        self._row_dtype = np.uint8 if self.cnn else np.float32
        self.n_actions = config.n_actions
        if config.ckpt_format != "tch":
            self._ckpt_ext = ".safetensors"

    def update_on_batch(self, obs, act, next_obs, reward, is_terminated, is_truncated=None) -> dict:
        """One Dqn::update_critic (dqn/base.rs:59-170) on host rows and opt_'s bookkeeping; act: int64 [n].  is_truncated is read by
        nothing, as in the reference.  The record: loss and, with record_verbose_level >= 2, the four means."""
        f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        obs, next_obs = (np.ascontiguousarray(x, dtype=self._row_dtype) for x in (obs, next_obs))
        reward = f(reward)
        n = len(reward)
        act = np.ascontiguousarray(act, dtype=np.int64).reshape(-1)
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        trunc = None if is_truncated is None else np.ascontiguousarray(is_truncated, dtype=np.int8)
        if obs.size != n * self.config.obs_dim or next_obs.size != obs.size or act.size != n or term.size != n:
            raise ValueError(f"rows must hold {n} x {self.config.obs_dim} observations and {n} actions, rewards and flags")
        rec = _lib.DqnRecordC()
        fn = _lib.lib().bdr_candle_dqn_cnn_update_on_batch if self.cnn else _lib.lib().bdr_candle_dqn_update_on_batch
        _lib.check(fn(self._h, n, _p(obs), _p(act), _p(next_obs), _p(reward), _p(term), _p(trunc), C.byref(rec)))
        out = {"loss": rec.loss}
        if rec.has_verbose:
            out.update(pred_mean=rec.pred_mean, reward_mean=rec.reward_mean, tgt_mean=rec.tgt_mean, tgt_minus_pred_mean=rec.tgt_minus_pred_mean)
        return out

    def probe(self, what: str, batch: int) -> np.ndarray:
        """Intermediates of the last update (bdr_candle_dqn_probe), each [B]: pred, q_next, y (the argmax index), tgt, dpred."""
        out = np.empty(batch, np.float32)
        _lib.check(_lib.lib().bdr_candle_dqn_probe(self._h, self.PROBES[what], _p(out), out.size))
        return out.astype(np.int64) if what == "y" else out

    # ---- Policy::sample (dqn/base.rs:202-230) ----
    def set_explorer(self, explorer: Union[Softmax, EpsilonGreedy], seed: int = 42) -> None:
        """DqnConfig::explorer; rewinds the exploration stream to SmallRng::seed_from_u64(seed)."""
        _lib.check(_lib.lib().bdr_agent_set_explorer(self._h, C.byref(explorer.to_c(seed))))

    def explorer_state(self) -> dict:
        e = _lib.ExplorerConfigC()
        _lib.check(_lib.lib().bdr_agent_get_explorer(self._h, C.byref(e)))
        return {"kind": "softmax" if e.kind == 0 else "eps_greedy", "eps_start": e.eps_start, "eps_final": e.eps_final,
                "final_step": e.final_step, "n_opts": e.n_calls}

    def sample(self, obs, return_info: bool = False):
        """float32 rows [n, obs_dim] (AtariCnn form: uint8 rows [n, 84 * 84 * n_stack]) -> int64 actions [n]"""
        obs = np.ascontiguousarray(obs, dtype=self._row_dtype).reshape(-1, self.config.obs_dim)
        a = np.empty(obs.shape[0], np.int64)
        info = _lib.SampleInfoC()
        _lib.check(_lib.lib().bdr_agent_sample(self._h, obs.shape[0], _p(obs), _p(a), C.byref(info)))
        return (a, _info(info)) if return_info else a

    def sample_device(self, obs_dev: int, n: int, row_stride: int, return_info: bool = False):
        a = np.empty(n, np.int64)
        info = _lib.SampleInfoC()
        _lib.check(_lib.lib().bdr_agent_sample_device(self._h, n, C.c_void_p(obs_dev), row_stride, _p(a), C.byref(info)))
        return (a, _info(info)) if return_info else a

    def _raw_out(self, n: int):
        return np.empty(n, np.int64), True   # DenseHandle.sample_raw / sample_raw_device: indices

    def qvalues(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs, dtype=self._row_dtype).reshape(-1, self.config.obs_dim)
        q = np.empty((obs.shape[0], self.n_actions), np.float32)
        _lib.check(_lib.lib().bdr_agent_qvalues(self._h, obs.shape[0], _p(obs), _p(q), None))
        return q

    def qvalues_device(self, obs_dev: int, n: int, row_stride: int) -> np.ndarray:
        q = np.empty((n, self.n_actions), np.float32)
        _lib.check(_lib.lib().bdr_agent_qvalues_device(self._h, n, C.c_void_p(obs_dev), row_stride, _p(q), None))
        return q

    def sample_greedy(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs, dtype=self._row_dtype).reshape(-1, self.config.obs_dim)
        a = np.empty(obs.shape[0], np.int64)
        _lib.check(_lib.lib().bdr_agent_qvalues(self._h, obs.shape[0], _p(obs), None, _p(a)))
        return a

    # ---- parameter views: the models are arenas of one layout, named as the tch Dqn names them ----
    def which(self, name: Optional[str] = None, role: str = "param") -> int:
        base = self.WHICH[name or self.SYNC_MODEL]
        if role == "param":
            return base
        if base != 0:
            raise ValueError("the optimizer state belongs to qnet")
        return {"grad": 4, "exp_avg": 2, "exp_avg_sq": 3}[role]
