"""Host-side mirror of border-tch-agent's Sac agent over the C ABI.

  SacConfig     border-tch-agent/src/sac/config.rs (defaults :85-105)
  EntCoefMode   border-tch-agent/src/sac/ent_coef.rs:14-25  (Fix(alpha) | Auto(target_entropy, lr))
  Sac           border-tch-agent/src/sac/base.rs (Agent, Policy::sample, SyncModel ships `pi` only)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .dqn import OptimizerConfig
from .handle import ROLES, AgentHandle, _p


@dataclass
class SacConfig:
    obs_dim: int = 0
    act_dim: int = 0
    pi_units: Tuple[int, ...] = (64, 64)        # ActorConfig.pi_config: MlpConfig(in, units, out)
    q_units: Tuple[int, ...] = (64, 64)         # CriticConfig.q_config
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    opt_actor: Optional[OptimizerConfig] = None   # ActorConfig.opt_config (sac/actor/config.rs:15); None = OptimizerConfig.Adam(lr_actor)
    opt_critic: Optional[OptimizerConfig] = None  # CriticConfig.opt_config; None = OptimizerConfig.Adam(lr_critic)
    gamma: float = 0.99
    tau: float = 0.005
    ent_coef_mode: tuple = ("Fix", 1.0)          # or ("Auto", target_entropy, lr)
    epsilon: float = 1e-4
    min_lstd: float = -20.0
    max_lstd: float = 2.0
    n_updates_per_opt: int = 1
    batch_size: int = 1
    train: bool = False
    critic_loss: str = "Mse"
    reward_scale: float = 1.0
    n_critics: int = 1
    seed: int = 0
    device: Optional[int] = None

    def to_c(self) -> _lib.SacConfigC:
        c = _lib.SacConfigC()
        _lib.lib().bdr_sac_config_default(C.byref(c))
        c.obs_dim, c.act_dim = self.obs_dim, self.act_dim
        c.n_pi_units, c.n_q_units = len(self.pi_units), len(self.q_units)
        for i, u in enumerate(self.pi_units):
            c.pi_units[i] = u
        for i, u in enumerate(self.q_units):
            c.q_units[i] = u
        c.lr_actor, c.lr_critic, c.gamma, c.tau = self.lr_actor, self.lr_critic, self.gamma, self.tau
        if self.ent_coef_mode[0] == "Auto":
            c.ent_coef_auto, c.target_entropy, c.ent_coef_lr = 1, self.ent_coef_mode[1], self.ent_coef_mode[2]
        else:
            c.ent_coef_auto, c.ent_coef_alpha = 0, self.ent_coef_mode[1]
        c.epsilon, c.min_lstd, c.max_lstd = self.epsilon, self.min_lstd, self.max_lstd
        c.n_updates_per_opt, c.batch_size, c.train = self.n_updates_per_opt, self.batch_size, int(self.train)
        c.critic_loss = {"Mse": 0, "SmoothL1": 1}[self.critic_loss]
        c.reward_scale, c.n_critics, c.seed = self.reward_scale, self.n_critics, self.seed
        c.device = -1 if self.device is None else self.device
        if self.opt_actor is not None:
            c.lr_actor = self.opt_actor.lr
            c.opt_actor.fill(self.opt_actor)
        if self.opt_critic is not None:
            c.lr_critic = self.opt_critic.lr
            c.opt_critic.fill(self.opt_critic)
        return c


class Sac(AgentHandle):
    """sac/base.rs; SyncModel ships only the policy network `pi` (:377-386)."""
    KIND = "sac"
    SYNC_MODEL = "pi"
    WHICH = {"qnet": 0, "pi": 0}   # ParamExchange / ModelMailbox: SyncModel ships `pi` == model 0
    CKPT_EXTS = {"tch": ".pt.tch", "safetensors": ".safetensors"}
    ROLES = {**ROLES, "max_exp_avg_sq": 400}   # AdamW{amsgrad}

    @property
    def CKPT_STEMS(self):   # sac/base.rs:313-334 order
        return [s for i in range(self.config.n_critics) for s in (f"qnet_{i}", f"qnet_tgt_{i}")] + ["pi", "ent_coef"]

    def _model_id(self, name: str) -> int:
        """pi 0, qnet_i 1 + i, qnet_tgt_i 1 + n_critics + i, log_alpha 1 + 2 n_critics"""
        nc = self.config.n_critics
        if name.startswith("qnet_tgt_"):
            return 1 + nc + int(name[len("qnet_tgt_"):])
        if name.startswith("qnet_"):
            return 1 + int(name[len("qnet_"):])
        return {"pi": 0, "log_alpha": 1 + 2 * nc}[name]

    # AgentHandle's parameter views under this class's own signatures: `pi` is the literal default, `which` needs a name
    def which(self, name: str, role: str = "param") -> int:
        return super().which(name, role)

    def arena_device_ptr(self, which="pi"):
        return super().arena_device_ptr(which)

    def param_count(self, name="pi") -> int:
        return super().param_count(name)

    def get_params(self, name="pi", role="param") -> np.ndarray:
        return super().get_params(name, role)

    def set_params(self, params, name="pi", role="param") -> None:
        super().set_params(params, name, role)

    def update_on_batch(self, obs, act, next_obs, reward, is_terminated, z_actor, z_next) -> dict:
        f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        obs, act, next_obs, reward, z_actor, z_next = map(f, (obs, act, next_obs, reward, z_actor, z_next))
        term = np.ascontiguousarray(is_terminated, dtype=np.int8)
        rec = np.zeros(3, np.float32)
        _lib.check(_lib.lib().bdr_sac_update_on_batch(self._h, len(reward), _p(obs), _p(act), _p(next_obs), _p(reward), _p(term),
                                                      _p(z_actor), _p(z_next), _p(rec)))
        return dict(loss_critic=float(rec[0]), loss_actor=float(rec[1]), ent_coef=float(rec[2]))

    PROBES = {"q_pred": 0, "q_next": 1, "qvals_min": 2, "next_log_p": 3, "tgt": 4, "q_pi": 5, "log_p": 6, "next_act": 7}

    def probe(self, what: str, batch: int) -> np.ndarray:
        """Intermediates of the last update (bdr_sac_probe): q_pred / q_next / q_pi [n_critics, B], qvals_min / next_log_p / tgt /
        log_p [B], next_act [B, act_dim]."""
        nc, ad = self.config.n_critics, self.config.act_dim
        shape = {"q_pred": (nc, batch), "q_next": (nc, batch), "q_pi": (nc, batch), "next_act": (batch, ad)}.get(what, (batch,))
        out = np.empty(shape, np.float32)
        _lib.check(_lib.lib().bdr_sac_probe(self._h, self.PROBES[what], _p(out), out.size))
        return out

    def keep_layers(self, on: bool = True) -> None:
        """bdr_sac_keep_layers: update_on_batch also keeps the actor phase's buffers aside (phase "actor" of `layer`).  Off by default."""
        _lib.check(_lib.lib().bdr_sac_keep_layers(self._h, int(bool(on))))

    PHASES = {"actor": 0, "critic": 1}   # BDR_SAC_PHASE_*
    BUFS = {"x_o": 0, "x_no": 1, "xq_a": 2, "xq_n": 3, "xq_c": 4, "z": 5, "t_act": 6, "t_dy": 7, "mean": 8, "e": 9, "a_s": 10, "s_s": 11,
            "sd_s": 12, "logp": 13, "gmean": 14, "ge": 15, "c_act": 16, "c2_act": 17, "c_dy": 18, "dxq": 19, "tgt": 20, "lrow": 21,
            "scal": 22, "log_alpha": 23, "pi_part": 24, "q_part": 25, "pi_grad": 26, "q_grad": 27, "pi_chunks": 28, "q_chunks": 29}   # BDR_SAC_BUF_*

    def layout(self, net: str):
        """Padded layers of `pi` (trunk, then the heads ml, sl) or `q`: a list of (in, out, Kp, Np, w, b) - sizes padded to 64, W [Kp][Np]
        at float offset w of the arena, bias [Np] at b (csrc/dense.hpp make_mlp)."""
        c, pad = self.config, lambda x: (x + 63) // 64 * 64
        if net == "pi":
            dims = [(i, o) for i, o in zip((c.obs_dim,) + tuple(c.pi_units[:-1]), c.pi_units)] + [(c.pi_units[-1], c.act_dim)] * 2
        else:
            dims = [(i, o) for i, o in zip((c.obs_dim + c.act_dim,) + tuple(c.q_units), tuple(c.q_units) + (1,))]
        out, o = [], 0
        for i, n in dims:
            kp, np_ = pad(i), pad(n)
            out.append((i, n, kp, np_, o, o + kp * np_))
            o += kp * np_ + np_
        return out

    def layer(self, buf: str, rows: int, phase: str = "critic", critic: int = 0, layer: int = 0) -> np.ndarray:
        """bdr_sac_layer_probe: one raw device buffer of the last update_on_batch (phase "critic" also: of the last `sample`), padding
        included; `rows` = the batch of that call.  Matrices come back [rows][ld]; z [2][rows][act_dim]; lrow [3 + n_critics][blocks];
        pi_part / q_part [chunks][Kp * Np + Np]; pi_grad / q_grad the flat padded arena; pi_chunks / q_chunks an int."""
        c = self.config
        pi, q = self.layout("pi"), self.layout("q")
        nt = len(c.pi_units)
        if buf in ("pi_chunks", "q_chunks"):
            out = np.zeros(1, np.float32)
            _lib.check(_lib.lib().bdr_sac_layer_probe(self._h, self.PHASES[phase], self.BUFS[buf], critic, layer, _p(out), 1))
            return int(out[0])
        if buf in ("x_o", "x_no"): shape = (rows, pi[0][2])
        elif buf in ("xq_a", "xq_n", "xq_c", "dxq"): shape = (rows, q[0][2])
        elif buf == "z": shape = (2, rows, c.act_dim)
        elif buf in ("t_act", "t_dy"): shape = (rows, pi[layer][3])
        elif buf in ("mean", "e", "a_s", "s_s", "sd_s", "gmean", "ge"): shape = (rows, pi[nt][3])
        elif buf in ("logp", "tgt"): shape = (rows,)
        elif buf in ("c_act", "c2_act", "c_dy"): shape = (rows, q[layer][3])
        elif buf == "lrow": shape = (3 + c.n_critics, (rows + 31) // 32)
        elif buf == "scal": shape = (4,)
        elif buf == "log_alpha": shape = (1,)
        elif buf == "pi_grad": shape = (pi[-1][5] + pi[-1][3],)
        elif buf == "q_grad": shape = (q[-1][5] + q[-1][3],)
        elif buf in ("pi_part", "q_part"):
            ly = (pi if buf == "pi_part" else q)[layer]
            shape = (self.layer(buf.replace("part", "chunks"), rows, phase, critic, layer), ly[2] * ly[3] + ly[3])
        else:
            raise KeyError(buf)
        out = np.empty(shape, np.float32)
        _lib.check(_lib.lib().bdr_sac_layer_probe(self._h, self.PHASES[phase], self.BUFS[buf], critic, layer, _p(out), out.size))
        return out

    def sample(self, obs) -> np.ndarray:
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        out = np.empty((obs.shape[0], self.config.act_dim), np.float32)
        _lib.check(_lib.lib().bdr_sac_sample(self._h, obs.shape[0], _p(obs), _p(out)))
        return out

    def sample_device(self, obs_dev: int, n: int, row_stride: int) -> np.ndarray:
        """`sample` for observation rows already in HBM (`bdr_sac_sample_device`): row i at obs_dev + i * row_stride bytes."""
        out = np.empty((n, self.config.act_dim), np.float32)
        _lib.check(_lib.lib().bdr_sac_sample_device(self._h, n, C.c_void_p(obs_dev), row_stride, _p(out)))
        return out
