"""DqnGroup: a set of small Mlp DQN agents whose Agent::opt runs as ONE launch, one workgroup per member (bdr_agent_group_*); so do
acting (`sample`) and pushing one transition per member (`push`), and `train` drives the three from a compiled online loop.

A launch grouping, not an agent kind: the members are ordinary `Dqn` objects (every `Dqn` method keeps working on a member and
means what it meant) that the group owns - `DqnGroup.close()` closes them, `member.close()` on a live group is refused.  Results
are bit for bit those of stepping the same agents one after the other.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .dqn import Dqn, DqnConfig, record_keys


class DqnGroup:
    STAGING_DEPTH = 8   # slots of the per-step staging ring (csrc/mlp_agents.hip bdr_agent_group::STEP_SLOTS)
    PUSH_STAGING_DEPTH = 8   # slots of the push staging ring (bdr_agent_group::PUSH_SLOTS)

    def __init__(self, agents, prioritized: bool = False):
        """Adopts already built `Dqn` agents (they must be Mlp agents that take the one-workgroup step; see bdr_agent_group_create).
        `prioritized=True`: opt / opt_with_record / push / train also accept buffers built with a `PerConfig`
        (bdr_agent_group_set_prioritized); by default a prioritized buffer is refused."""
        agents = list(agents)
        hs = (C.c_void_p * len(agents))(*[a.handle for a in agents])
        g = C.c_void_p()
        _lib.check(_lib.lib().bdr_agent_group_create(hs, len(agents), C.byref(g)))
        self._g = g
        self._members = agents
        self._keys = None
        self._bound = None   # the handle array of the buffers passed last (opt() without an argument steps on them again)
        dims = {a.config.model_config.q_config.in_dim for a in agents}
        self._in_dim = dims.pop() if len(dims) == 1 else None   # one input width for all: sample / qvalues also take a [n, in_dim] array
        self._prioritized = False
        if prioritized:
            try:
                self.set_prioritized(True)
            except Exception:
                _lib.lib().bdr_agent_group_destroy(g)   # (destroys the adopted members)
                self._g = None
                for a in agents:
                    a._h = None
                raise

    @classmethod
    def build(cls, configs, prioritized: bool = False) -> "DqnGroup":
        """One `Dqn` per DqnConfig, grouped.  Nothing is left behind when a config is refused."""
        agents = []
        try:
            for c in configs:
                agents.append(Dqn.build(c))
            return cls(agents, prioritized=prioritized)
        except Exception:
            for a in agents:
                a.close()
            raise

    @property
    def members(self):
        return list(self._members)

    def __len__(self):
        return len(self._members)

    @property
    def prioritized(self) -> bool:
        return self._prioritized

    def set_prioritized(self, on: bool) -> None:
        """Switches prioritized replay under the group on or off (bdr_agent_group_set_prioritized): on, the prioritized members' tree
        sampling, weights and priority updates run as a fixed number of launches per round, bit for bit what their own calls give."""
        _lib.check(_lib.lib().bdr_agent_group_set_prioritized(self._g, 1 if on else 0))
        self._prioritized = bool(on)

    @property
    def handle(self):
        return self._g

    def _buffers(self, buffers):
        if buffers is None:   # the buffers of the last call (building the handle array costs ~0.2 us per member in Python)
            if self._bound is None:
                raise ValueError("opt() without buffers needs an earlier call that named them")
            return self._bound
        buffers = list(buffers)
        if len(buffers) != len(self._members):
            raise ValueError(f"{len(self._members)} members need {len(self._members)} buffers, got {len(buffers)}")
        self._bound = (C.c_void_p * len(buffers))(*[b.handle for b in buffers])
        return self._bound

    def opt(self, buffers=None) -> None:
        """Agent::opt of every member on its own buffer: n_updates_per_opt launches in all; does not synchronise.
        `buffers=None`: the buffers of the last opt / opt_with_record call (they must still be open)."""
        _lib.check(_lib.lib().bdr_agent_group_opt(self._g, self._buffers(buffers)))

    def opt_with_record(self, buffers=None) -> list:
        """Agent::opt_with_record of every member (one synchronisation): a list of Record dicts in member order."""
        n, cap = len(self._members), 128
        out = np.zeros((n, cap), np.float32)
        cnt = np.zeros(n, np.int32)
        _lib.check(_lib.lib().bdr_agent_group_opt_with_scalars(self._g, self._buffers(buffers), out.ctypes.data_as(C.c_void_p), cap,
                                                               cnt.ctypes.data_as(C.c_void_p)))
        if self._keys is None:
            self._keys = [record_keys(a.handle) for a in self._members]
        return [{k: float(v) for k, v in zip(self._keys[i], out[i, :cnt[i]])} for i in range(n)]

    def _rows(self, rows):
        n = len(self._members)
        if isinstance(rows, np.ndarray) and self._in_dim is not None and rows.dtype == np.float32 and rows.shape == (n, self._in_dim) \
                and rows.flags.c_contiguous:   # one array for all members: row addresses by arithmetic, no per-row objects
            ptrs = np.uint64(rows.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(4 * self._in_dim)
            return rows, ptrs.ctypes.data_as(C.c_void_p), ptrs
        rows = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1) for r in rows]
        if len(rows) != len(self._members):
            raise ValueError(f"{len(self._members)} members need {len(self._members)} observation rows, got {len(rows)}")
        for i, (r, a) in enumerate(zip(rows, self._members)):
            want = a.config.model_config.q_config.in_dim
            if r.size != want:
                raise ValueError(f"member {i}: an observation row of {want} f32, got {r.size}")
        return rows, (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows]), None

    def qvalues(self, rows) -> list:
        """qnet.forward of one observation row per member, one launch: a list of [A_i] float32 arrays."""
        rows, ptrs, _keep = self._rows(rows)
        qs = [np.empty(a.n_actions, np.float32) for a in self._members]
        outs = (C.c_void_p * len(qs))(*[q.ctypes.data for q in qs])
        _lib.check(_lib.lib().bdr_agent_group_qvalues(self._g, ptrs, outs))
        return qs

    def sample(self, rows, return_info: bool = False):
        """Policy::sample of every member on one observation row each, one launch: int64 actions [n] (and the per-member info).
        rows: one row per member, or - when every member has the same in_dim - a float32 array [n, in_dim]."""
        rows, ptrs, _keep = self._rows(rows)
        n = len(rows)
        act = np.empty(n, np.int64)
        info = (_lib.SampleInfoC * n)()
        _lib.check(_lib.lib().bdr_agent_group_sample(self._g, ptrs, act.ctypes.data_as(C.c_void_p), info))
        if return_info:
            return act, [{"eps": i.eps, "is_random": bool(i.is_random), "n_samples_act": i.n_samples_act,
                          "n_samples_best_act": i.n_samples_best_act} for i in info]
        return act

    def push(self, obs, act, next_obs, reward, is_terminated, is_truncated, buffers=None) -> None:
        """ExperienceBufferBase::push of one transition per member into the member's own buffer, one launch; does not synchronise.
        obs / next_obs: one row per member, or a float32 array [n, in_dim] when every member has the same in_dim; act [n] (or [n, 1])
        int64, reward [n] float32, the flags [n] int8.  `buffers=None`: the buffers named last (as opt())."""
        bufs = self._buffers(buffers)
        n = len(self._members)
        _o, optrs, _ko = self._rows(obs)
        _x, xptrs, _kx = self._rows(next_obs)
        act = np.ascontiguousarray(act, np.int64).reshape(-1)
        reward = np.ascontiguousarray(reward, np.float32).reshape(-1)
        term = np.ascontiguousarray(is_terminated, np.int8).reshape(-1)
        trunc = np.ascontiguousarray(is_truncated, np.int8).reshape(-1)
        for name, a in (("act", act), ("reward", reward), ("is_terminated", term), ("is_truncated", trunc)):
            if a.size != n:
                raise ValueError(f"{n} members need {n} values of {name}, got {a.size}")
        _lib.check(_lib.lib().bdr_agent_group_push(self._g, bufs, optrs, act.ctypes.data_as(C.c_void_p), xptrs, reward.ctypes.data_as(C.c_void_p),
                                                   term.ctypes.data_as(C.c_void_p), trunc.ctypes.data_as(C.c_void_p)))

    def train(self, envs, buffers, trainer_config, on_event=None) -> list:
        """The compiled online loop over the group (bdr_trainer_train_group): member i on envs[i] and buffers[i], one group sample,
        one group push and at most one group opt per iteration.  on_event(member, env_steps, opt_steps, event, scalars); returns one
        statistics dict per member."""
        from .trainer import NativeTrainer
        self._buffers(buffers)   # (opt() / push() without buffers go on with these)
        return NativeTrainer(trainer_config).train_group(envs, self, list(buffers), on_event=on_event)

    def sync(self) -> None:
        _lib.check(_lib.lib().bdr_agent_group_sync(self._g))

    def close(self) -> None:
        if getattr(self, "_g", None):
            _lib.check(_lib.lib().bdr_agent_group_destroy(self._g))   # destroys the members
            self._g = None
            for a in self._members:
                a._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
