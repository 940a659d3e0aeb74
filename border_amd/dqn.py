"""Host-side mirror of border-tch-agent's Dqn agent over the C ABI.

Same names / argument meaning as the reference:
  DqnConfig        border-tch-agent/src/dqn/config.rs:26-48 (defaults :82-102)
  DqnModelConfig   border-tch-agent/src/dqn/model/config.rs (q_config + opt_config)
  AtariCnnConfig   border-tch-agent/src/cnn/config.rs:13-18
  OptimizerConfig  border-tch-agent/src/opt.rs:13-28
  Dqn              border-tch-agent/src/dqn/base.rs  (Agent: train/eval/is_train/opt/
                   opt_with_record/save_params/load_params; Policy::sample; SyncModel)
All arithmetic runs in the HIP library; there is no CPU fallback here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .handle import AgentHandle, _p, draw_noise, opt_with_named_record, record_keys  # noqa: F401  (the helpers: importable from here as before)


@dataclass
class AtariCnnConfig:
    n_stack: int = 4
    out_dim: int = 0
    skip_linear: bool = False


@dataclass
class MlpConfig:
    in_dim: int = 0
    units: Tuple[int, ...] = ()
    out_dim: int = 0
    activation_out: bool = False


@dataclass
class OptimizerConfig:
    """opt.rs:13-28: Adam{lr} or AdamW{lr,beta1,beta2,wd,eps,amsgrad}."""
    kind: str = "Adam"
    lr: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    wd: float = 0.0
    eps: float = 1e-8
    amsgrad: bool = False

    @classmethod
    def Adam(cls, lr: float) -> "OptimizerConfig":
        return cls("Adam", lr)

    @classmethod
    def AdamW(cls, lr: float, beta1: float = 0.9, beta2: float = 0.999, wd: float = 0.01, eps: float = 1e-8,
              amsgrad: bool = False) -> "OptimizerConfig":
        return cls("AdamW", lr, beta1, beta2, wd, eps, amsgrad)


@dataclass
class Softmax:
    """dqn/explorer.rs:17-32 (the DqnConfig default, dqn/config.rs:93)."""

    def to_c(self, seed: int = 0) -> "_lib.ExplorerConfigC":
        e = _lib.ExplorerConfigC()
        _lib.lib().bdr_explorer_config_default(C.byref(e), 0)
        e.seed = seed
        return e


@dataclass
class EpsilonGreedy:
    """dqn/explorer.rs:34-120: eps decays linearly over `final_step` action() calls."""
    n_opts: int = 0
    eps_start: float = 1.0
    eps_final: float = 0.02
    final_step: int = 100_000

    @classmethod
    def with_final_step(cls, final_step: int) -> "EpsilonGreedy":
        return cls(final_step=final_step)

    def to_c(self, seed: int = 0) -> "_lib.ExplorerConfigC":
        e = _lib.ExplorerConfigC()
        _lib.lib().bdr_explorer_config_default(C.byref(e), 1)
        e.eps_start, e.eps_final, e.final_step, e.n_calls, e.seed = self.eps_start, self.eps_final, self.final_step, self.n_opts, seed
        return e


@dataclass
class DqnModelConfig:
    q_config: Optional[object] = None
    opt_config: OptimizerConfig = field(default_factory=lambda: OptimizerConfig.Adam(0.0))


@dataclass
class DqnConfig:
    """dqn/config.rs:26-48 with the defaults of :82-102."""
    model_config: DqnModelConfig = field(default_factory=DqnModelConfig)
    soft_update_interval: int = 1
    n_updates_per_opt: int = 1
    batch_size: int = 1
    discount_factor: float = 0.99
    tau: float = 0.005
    train: bool = False
    clip_reward: Optional[float] = None     # never used by the reference either (dqn/base.rs:42,276)
    double_dqn: bool = False
    clip_td_err: Optional[Tuple[float, float]] = None
    device: Optional[int] = None            # None -> "No device is given for DQN agent" (dqn/base.rs:256)
    critic_loss: str = "Mse"                # util.rs:17-23
    record_verbose_level: int = 0
    param_seed: int = 0
    arithmetic: str = "bf16x3_6"            # BDR_ARITH_* (include/border_amd.h; not a reference field): "bf16x3_6" | "f32_exact"

    def to_c(self) -> _lib.DqnConfigC:
        c = _lib.DqnConfigC()
        _lib.lib().bdr_dqn_config_default(C.byref(c))
        q = self.model_config.q_config
        if isinstance(q, AtariCnnConfig):
            if q.skip_linear:
                raise NotImplementedError("skip_linear AtariCnn is only used by IQN (not built yet)")
            c.net.kind, c.net.n_stack, c.net.out_dim = 0, q.n_stack, q.out_dim
        elif isinstance(q, MlpConfig):
            c.net.kind, c.net.in_dim, c.net.n_units, c.net.out_dim = 1, q.in_dim, len(q.units), q.out_dim
            for i, u in enumerate(q.units):
                c.net.units[i] = u
            c.net.activation_out = int(q.activation_out)
        else:
            raise ValueError("model_config.q_config must be an AtariCnnConfig or MlpConfig")
        o = self.model_config.opt_config
        c.opt_kind = {"Adam": 0, "AdamW": 1}[o.kind]
        c.lr, c.beta1, c.beta2, c.weight_decay, c.eps = o.lr, o.beta1, o.beta2, o.wd, o.eps
        c.amsgrad = 1 if (o.kind == "AdamW" and o.amsgrad) else 0
        c.soft_update_interval, c.n_updates_per_opt, c.batch_size = (self.soft_update_interval,
                                                                    self.n_updates_per_opt, self.batch_size)
        c.discount_factor, c.tau, c.train = self.discount_factor, self.tau, int(self.train)
        c.double_dqn = int(self.double_dqn)
        c.critic_loss = {"Mse": 0, "SmoothL1": 1}[self.critic_loss]
        if self.clip_td_err is not None:
            c.has_clip_td_err, (c.clip_td_err_min, c.clip_td_err_max) = 1, self.clip_td_err
        c.record_verbose_level = self.record_verbose_level
        c.device = -1 if self.device is None else self.device
        c.param_seed = self.param_seed
        c.arithmetic = _lib.ARITHMETIC[self.arithmetic]
        return c


def _sample_info(info) -> dict:
    return {"eps": info.eps, "is_random": bool(info.is_random), "n_samples_act": info.n_samples_act, "n_samples_best_act": info.n_samples_best_act}


class TchValueAgent(AgentHandle):
    """What the handles of the tch Dqn and Iqn share on AgentHandle: their arenas are MODELS 0..5 named by WHICH (no roles), their files
    are `<stem>.pt.tch` archives, and Policy::sample returns int64 actions from the library's exploration stream."""
    CKPT_EXTS = {"tch": ".pt.tch", "safetensors": ".safetensors"}

    def param_count(self) -> int:
        n = C.c_uint64()
        _lib.check(_lib.lib().bdr_agent_param_count(self._h, C.byref(n)))
        return n.value

    def get_params(self, which) -> np.ndarray:
        out = np.empty(self.param_count(), np.float32)
        _lib.check(_lib.lib().bdr_agent_get_params(self._h, self.WHICH[which], _p(out), out.size))
        return out

    def set_params(self, params: np.ndarray, which) -> None:
        p = np.ascontiguousarray(params, dtype=np.float32)
        _lib.check(_lib.lib().bdr_agent_set_params(self._h, self.WHICH[which], _p(p), p.size))

    def set_explorer(self, explorer: "Softmax | EpsilonGreedy", seed: int = 0) -> None:
        """DqnConfig::explorer (dqn/config.rs:45), IqnConfig::explorer (iqn/config.rs:35; default Softmax); `seed` seeds the library's
        exploration stream."""
        _lib.check(_lib.lib().bdr_agent_set_explorer(self._h, C.byref(explorer.to_c(seed))))

    def sample(self, obs, return_info: bool = False):
        """Policy::sample (dqn/base.rs:211-242, iqn/base.rs:204-228): forward on the device + the configured exploration (train) /
        argmax (eval).  obs: [n_procs, ...] rows as stored in the replay buffer; returns int64 actions [n_procs]."""
        obs = np.ascontiguousarray(obs)
        a = np.empty(obs.shape[0], np.int64)
        info = _lib.SampleInfoC()
        _lib.check(_lib.lib().bdr_agent_sample(self._h, obs.shape[0], _p(obs), _p(a), C.byref(info)))
        return (a, _sample_info(info)) if return_info else a

    def sample_device(self, obs_dev: int, n: int, row_stride: int, return_info: bool = False):
        """Policy::sample for observation rows already in HBM (`bdr_agent_sample_device`): row i at obs_dev + i * row_stride bytes."""
        a = np.empty(n, np.int64)
        info = _lib.SampleInfoC()
        _lib.check(_lib.lib().bdr_agent_sample_device(self._h, n, C.c_void_p(obs_dev), row_stride, _p(a), C.byref(info)))
        return (a, _sample_info(info)) if return_info else a

    def qvalues_device(self, obs_dev: int, n: int, row_stride: int) -> np.ndarray:
        q = np.empty((n, self.n_actions), np.float32)
        _lib.check(_lib.lib().bdr_agent_qvalues_device(self._h, n, C.c_void_p(obs_dev), row_stride, _p(q), None))
        return q


class Dqn(TchValueAgent):
    """Dqn<E, Q, R> (dqn/base.rs:22-48); Configurable::build (:252-286); checkpoints qnet, qnet_tgt (:348-356); SyncModel ships
    qnet (:377-402)."""
    KIND = "dqn"
    CKPT_STEMS = ("qnet", "qnet_tgt")
    SYNC_MODEL = "qnet"
    WHICH = {"qnet": 0, "qnet_tgt": 1, "exp_avg": 2, "exp_avg_sq": 3, "grad": 4, "max_exp_avg_sq": 5}

    def __init__(self, config: DqnConfig):
        super().__init__(config)
        self.n_actions = config.model_config.q_config.out_dim

    def close(self):
        if getattr(self, "_h", None):
            _lib.check(_lib.lib().bdr_agent_destroy(self._h))   # (refused for a member of a live DqnGroup: the group owns it)
            self._h = None

    # the parameter views under this class's own signatures: `qnet` is the literal default
    def arena_device_ptr(self, which="qnet"):
        return super().arena_device_ptr(which)

    def get_params(self, which="qnet") -> np.ndarray:
        return super().get_params(which)

    def set_params(self, params: np.ndarray, which="qnet") -> None:
        super().set_params(params, which)

    @staticmethod
    def _record(r) -> dict:
        rec = {"loss": r.loss}
        if r.has_verbose:
            rec.update(pred_mean=r.pred_mean, reward_mean=r.reward_mean, tgt_mean=r.tgt_mean,
                       tgt_minus_pred_mean=r.tgt_minus_pred_mean)
        return rec

    def update_on_batch(self, obs, act, next_obs, reward, is_terminated, weight=None) -> dict:
        """One Dqn::opt_ on a caller-supplied minibatch (fixed-minibatch parity tests).  With `weight` the
        importance-weighted branch of update_critic runs (dqn/base.rs:123-145) and the record carries `td_errs`."""
        reward = np.ascontiguousarray(reward, dtype=np.float32)
        n = len(reward)
        obs, next_obs = np.ascontiguousarray(obs), np.ascontiguousarray(next_obs)
        act = np.ascontiguousarray(act, dtype=np.int64).reshape(n)
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        r = _lib.DqnRecordC()
        if weight is None:
            _lib.check(_lib.lib().bdr_dqn_update_on_batch(self._h, n, _p(obs), _p(act), _p(next_obs), _p(reward), _p(term),
                                                          C.byref(r)))
            return self._record(r)
        w = np.ascontiguousarray(weight, dtype=np.float32)
        td = np.empty(n, np.float32)
        _lib.check(_lib.lib().bdr_dqn_update_on_batch_weighted(self._h, n, _p(obs), _p(act), _p(next_obs), _p(reward), _p(term),
                                                               _p(w), _p(td), C.byref(r)))
        rec = self._record(r)
        rec["td_errs"] = td
        return rec

    def grads_on_batch(self, obs, act, next_obs, reward, is_terminated) -> dict:
        """update_critic up to loss.backward() on a host minibatch: gradients -> get_params("grad"); nothing else changes."""
        reward = np.ascontiguousarray(reward, dtype=np.float32)
        n = len(reward)
        obs, next_obs = np.ascontiguousarray(obs), np.ascontiguousarray(next_obs)
        act = np.ascontiguousarray(act, dtype=np.int64).reshape(n)
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        r = _lib.DqnRecordC()
        _lib.check(_lib.lib().bdr_dqn_grads_on_batch(self._h, n, _p(obs), _p(act), _p(next_obs), _p(reward), _p(term), C.byref(r)))
        return self._record(r)

    def apply_grads(self) -> None:
        """The optimizer step on the gradient arena + opt_'s bookkeeping (soft update counter, n_opts)."""
        _lib.check(_lib.lib().bdr_agent_apply_grads(self._h))

    def explorer_state(self) -> dict:
        e = _lib.ExplorerConfigC()
        _lib.check(_lib.lib().bdr_agent_get_explorer(self._h, C.byref(e)))
        return {"kind": "softmax" if e.kind == 0 else "eps_greedy", "eps_start": e.eps_start, "eps_final": e.eps_final,
                "final_step": e.final_step, "n_opts": e.n_calls}

    def qvalues(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs)
        n = obs.shape[0]
        q = np.empty((n, self.n_actions), np.float32)
        _lib.check(_lib.lib().bdr_agent_qvalues(self._h, n, _p(obs), _p(q), None))
        return q

    def sample_greedy(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs)
        n = obs.shape[0]
        a = np.empty(n, np.int64)
        _lib.check(_lib.lib().bdr_agent_qvalues(self._h, n, _p(obs), None, _p(a)))
        return a

    def arena_release(self, which="qnet") -> None:
        """hands an arena back after arena_device_ptr: the library's derived copies (bf16 weight planes) are trusted again"""
        _lib.check(_lib.lib().bdr_agent_arena_release(self._h, self.WHICH[which]))

    def probe(self, what: str, n: int) -> np.ndarray:
        idx = {"q_pred_all": 0, "q_next_all": 1, "pred": 2, "tgt": 3, "loss": 4, "act_conv1": 5, "act_conv2": 6, "act_conv3": 7,
               "h1": 8, "dq": 9, "dh1": 10, "dy3": 11, "dy2": 12, "dy1": 13,   # 8-13 AtariCnn only: the backward pass's inputs and intermediates
               # AtariCnn only: qnet_tgt(next_obs) (its Q rows: q_next_all) and, with double DQN, qnet(next_obs)
               "tgt_conv1": 14, "tgt_conv2": 15, "tgt_conv3": 16, "tgt_h1": 17,
               "sel_conv1": 18, "sel_conv2": 19, "sel_conv3": 20, "sel_h1": 21, "q_sel_all": 22}[what]
        out = np.empty(n, np.float32)
        _lib.check(_lib.lib().bdr_dqn_probe(self._h, idx, _p(out), n))
        return out

    BUFS = {"x_in": 0, "act": 1, "dy": 2, "pred": 3, "tgt": 4, "loss_row": 5, "td_abs": 6, "loss": 7, "dw_part": 8, "q": 9, "q_tgt": 10,
            "grad": 11, "m": 12, "v": 13, "chunks": 14, "form": 15}   # BDR_DQN_MLP_BUF_*
    FORMS = ("lds", "global", "layers_head", "layers_td", "tiles")     # BDR_DQN_MLP_FORM_*

    def layer(self, buf: str, rows: int, z: int = 0, layer: int = 0):
        """bdr_dqn_mlp_layer_probe (Mlp Q-network only): one raw device buffer of the last update, padding included.  `rows` is that
        update's batch size; the library refuses any other float count.  x_in, act, dy: [rows][padded width]; pred, tgt, loss_row,
        td_abs: [rows]; loss: [1]; dw_part: [chunks][Kp * Np + Np]; q, q_tgt, grad, m, v: the whole padded arena; chunks: int."""
        q = self.config.model_config.q_config
        if not isinstance(q, MlpConfig):
            raise TypeError("Dqn.layer reads the buffers of an Mlp Q-network")
        pad = lambda x: (x + 63) // 64 * 64
        widths = (q.in_dim,) + tuple(q.units) + (q.out_dim,)
        Kp, Np = [pad(w) for w in widths[:-1]], [pad(w) for w in widths[1:]]
        if buf in ("chunks", "form"):
            out = np.empty(1, np.float32)
            _lib.check(_lib.lib().bdr_dqn_mlp_layer_probe(self._h, self.BUFS[buf], z, layer, _p(out), 1))
            return int(out[0])
        if buf in ("act", "dy", "dw_part") and not 0 <= layer < len(Np):
            raise IndexError("layer %d of %d" % (layer, len(Np)))
        total = sum(k * n + n for k, n in zip(Kp, Np))
        if buf == "dw_part":
            shape = (self.layer("chunks", rows), Kp[layer] * Np[layer] + Np[layer])
        else:
            shape = {"x_in": (rows, Kp[0]), "act": (rows, Np[layer]), "dy": (rows, Np[layer]), "pred": (rows,), "tgt": (rows,),
                     "loss_row": (rows,), "td_abs": (rows,), "loss": (1,), "q": (total,), "q_tgt": (total,), "grad": (total,),
                     "m": (total,), "v": (total,)}[buf]
        out = np.empty(shape, np.float32)
        _lib.check(_lib.lib().bdr_dqn_mlp_layer_probe(self._h, self.BUFS[buf], z, layer, _p(out), out.size))
        return out

    @property
    def step_form(self) -> str:
        """the step the last update took: one of FORMS"""
        return self.FORMS[self.layer("form", 0)]

    def profile_read(self) -> dict:
        """{bracket name: mean milliseconds} (AgentHandle.profile_read as a dict)"""
        return dict(super().profile_read())
