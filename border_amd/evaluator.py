"""The Evaluator of the Trainer loops over the C ABI (csrc/trainer.hip: bdr_evaluate).

  Evaluator     border-core/src/evaluator/default_evaluator.rs:64-88 and border-minari/src/evaluator.rs:25-62: n_episodes episodes, one
                after the other, from env.reset_with_index(ix); the score is the f32 sum of all rewards, in call order, divided by
                n_episodes; with reference scores also (score - min) / (max - min) (border-minari/src/env.rs:162-168).
  EvalResult    what one evaluation returns.

`env` is any object with reset_with_index(ix) -> one observation row and step(act) -> (obs, reward, is_terminated, is_truncated).
Rows of `obs_dtype` float64 (Minari environments) or rows that need `obs_norm` reach the agent through bdr_agent_sample_raw (IQL,
AWAC, BC): rounded to float32 and normalised on the device.  The loop itself runs in compiled code; it does not switch the agent's
train / eval mode - the Trainer does (trainer.rs:246-248).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _lib


@dataclass
class EvalResult:
    score: float                 # np.float32 value of r_total / n_episodes
    normalized: Optional[float]  # None without reference scores
    n_steps: int
    n_episodes: int


class Evaluator:
    def __init__(self, env, n_episodes: int, obs_norm=None, obs_dtype=np.float32, ref_scores: Optional[Tuple[float, float]] = None,
                 obs_dim: Optional[int] = None, act_dim: int = 1, act_dtype=np.float32):
        """obs_dim: elements of one observation row (default: the normaliser's dim); act_dim / act_dtype: the action row the agent's
        Policy::sample writes (f32 rows of act_dim, or one i64 for discrete agents)."""
        self.env, self.n_episodes, self.obs_norm = env, int(n_episodes), obs_norm
        self.obs_dtype, self.act_dtype = np.dtype(obs_dtype), np.dtype(act_dtype)
        if self.obs_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("obs_dtype must be float32 or float64")
        if obs_dim is None:
            if obs_norm is None:
                raise ValueError("obs_dim is needed without a normaliser")
            obs_dim = obs_norm.dim
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.ref_scores = ref_scores
        self.error: Optional[BaseException] = None   # an exception raised by env inside a callback (the call then fails with status 99)
        self._c = None

    # the C view: built once, kept alive with its callbacks
    def c_struct(self) -> "_lib.EvaluatorC":
        if self._c is not None:
            return self._c
        row = self.obs_dim * self.obs_dtype.itemsize
        act_bytes = self.act_dim * self.act_dtype.itemsize

        def write(ptr, obs):
            C.memmove(ptr, np.ascontiguousarray(obs, self.obs_dtype).reshape(-1).ctypes.data, row)

        def reset(_ctx, ix, obs_out):
            try:
                write(obs_out, self.env.reset_with_index(int(ix)))
                return 0
            except BaseException as e:  # noqa: BLE001  (an exception cannot cross the C frame: it becomes a status)
                self.error = e
                return 99

        def step(_ctx, act, obs_out, reward, term, trunc):
            try:
                a = np.frombuffer((C.c_char * act_bytes).from_address(act), self.act_dtype).copy()
                obs, r, t, tr = self.env.step(a)
                write(obs_out, obs)
                reward[0], term[0], trunc[0] = float(r), int(bool(t)), int(bool(tr))
                return 0
            except BaseException as e:  # noqa: BLE001
                self.error = e
                return 99

        ev = _lib.EvaluatorC()
        _lib.lib().bdr_evaluator_default(C.byref(ev), None)
        ev.n_episodes, ev.obs_row_bytes, ev.act_row_bytes = self.n_episodes, row, act_bytes
        ev.obs_dtype = _lib.BDR_DTYPE_F32 if self.obs_dtype == np.float32 else _lib.BDR_DTYPE_F64
        ev.norm = self.obs_norm.handle if self.obs_norm is not None else None
        if self.ref_scores is not None:
            ev.has_ref_scores, ev.ref_min_score, ev.ref_max_score = 1, float(self.ref_scores[0]), float(self.ref_scores[1])
        self._keep = (_lib.EVAL_RESET_FN(reset), _lib.EVAL_STEP_FN(step))
        ev.env = _lib.EvalEnvVtable(None, *self._keep, 0, 0)
        self._c = ev
        return ev

    def _raise(self, status: int):
        if status == 99 and self.error is not None:
            e, self.error = self.error, None
            raise e
        _lib.check(status)

    def evaluate(self, agent) -> EvalResult:
        """One evaluation of `agent` (a handle class of this package) in the mode it is in."""
        out = _lib.EvalResultC()
        self._raise(_lib.lib().bdr_evaluate(C.byref(self.c_struct()), agent.handle, C.byref(out)))
        return EvalResult(np.float32(out.score), np.float32(out.normalized) if out.has_normalized else None, out.n_steps, out.n_episodes)
