"""Episode datasets -> replay ring, and the observation normalisation that goes with them.

Host-side mirror of
  MinariDataset::create_replay_buffer            border-minari/src/dataset.rs:64-109
  PenConverter::{new, convert_observation, ...}  border-minari/src/d4rl/pen/candle.rs:42-161
over the C ABI (`bdr_obs_norm_*`, `bdr_replay_push_episode`, `bdr_replay_summarize`).  An episode is anything with
`observations` ([T + 1, dim]; float64 in Minari's files), `actions`, `rewards`, `terminations`, `truncations` ([T]) as
attributes or keys - what `minari`'s `iterate_episodes()` yields.  `minari` itself is never imported.
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib
from .replay import SimpleReplayBuffer, SimpleReplayBufferConfig, _p

log = logging.getLogger(__name__)

EPISODE_FIELDS = ("observations", "actions", "rewards", "terminations", "truncations")


def _field(ep, name):
    return ep[name] if isinstance(ep, dict) else getattr(ep, name)


def episode_arrays(ep, obs_key: Optional[str] = None):
    """(observations [T + 1, dim], actions [T, ...], rewards [T], terminations [T], truncations [T]) of one episode.  `obs_key`
    picks one entry of a dict observation (kitchen, antmaze, pointmaze: "observation").  float32 observations stay float32, every
    other dtype becomes float64 (the dtype Minari stores)."""
    obs = _field(ep, "observations")
    if obs_key is not None:
        obs = obs[obs_key]
    obs = np.asarray(obs)
    if obs.dtype != np.float32:
        obs = obs.astype(np.float64, copy=False)
    obs = np.ascontiguousarray(obs).reshape(obs.shape[0], -1)
    rewards = np.asarray(_field(ep, "rewards")).reshape(-1)
    if obs.shape[0] != rewards.shape[0] + 1:
        raise ValueError(f"an episode of {rewards.shape[0]} transitions has {rewards.shape[0] + 1} observation rows, not {obs.shape[0]}")
    return obs, np.asarray(_field(ep, "actions")), rewards, np.asarray(_field(ep, "terminations")), np.asarray(_field(ep, "truncations"))


def _dtype_code(a: np.ndarray) -> int:
    return _lib.BDR_DTYPE_F32 if a.dtype == np.float32 else _lib.BDR_DTYPE_F64


class ObsNormalizer:
    """PenConverter's mean / std and `(x.astype(float32) - mean) / std` (pen/candle.rs:42-74).  The statistics are accumulated on
    the device in float64 over the float32-rounded rows, in a fixed order, and rounded to float32 once; `apply` (host) and
    `apply_device` (HBM) give the same bits as the rows `SimpleReplayBuffer.push_episode` writes."""

    def __init__(self, dim: int, device: int = 0):
        self.dim, self.device = int(dim), device
        h = C.c_void_p()
        _lib.check(_lib.lib().bdr_obs_norm_create(device, self.dim, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().bdr_obs_norm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _rows(self, rows) -> np.ndarray:
        rows = np.asarray(rows)
        if rows.dtype != np.float32:
            rows = rows.astype(np.float64, copy=False)
        rows = np.ascontiguousarray(rows).reshape(-1, self.dim)
        return rows

    # statistics -----------------------------------------------------------------------------
    def accumulate(self, rows) -> "ObsNormalizer":
        """The rows that count: the first T observation rows of an episode (the reference drops the last one, pen/candle.rs:56)."""
        rows = self._rows(rows)
        _lib.check(_lib.lib().bdr_obs_norm_accumulate(self._h, rows.shape[0], _p(rows), _dtype_code(rows)))
        return self

    def finish(self) -> "ObsNormalizer":
        _lib.check(_lib.lib().bdr_obs_norm_finish(self._h))
        return self

    def set(self, mean, std) -> "ObsNormalizer":
        mean = np.ascontiguousarray(mean, np.float32).reshape(self.dim)
        std = np.ascontiguousarray(std, np.float32).reshape(self.dim)
        _lib.check(_lib.lib().bdr_obs_norm_set(self._h, _p(mean), _p(std)))
        return self

    @classmethod
    def from_episodes(cls, episodes: Iterable, obs_key: Optional[str] = None, device: int = 0) -> "ObsNormalizer":
        """PenConverter::new: statistics over observations[:-1] of every episode."""
        self = None
        for ep in episodes:
            obs = episode_arrays(ep, obs_key)[0]
            if self is None:
                self = cls(obs.shape[1], device)
            self.accumulate(obs[:-1])
        if self is None:
            raise ValueError("no episodes")
        return self.finish()

    def _get(self):
        mean, std, n = np.empty(self.dim, np.float32), np.empty(self.dim, np.float32), C.c_uint64()
        _lib.check(_lib.lib().bdr_obs_norm_get(self._h, _p(mean), _p(std), C.byref(n)))
        return mean, std, n.value

    @property
    def mean(self) -> np.ndarray:
        return self._get()[0]

    @property
    def std(self) -> np.ndarray:
        return self._get()[1]

    @property
    def count(self) -> int:
        return self._get()[2]

    # convert_observation --------------------------------------------------------------------
    def apply(self, rows) -> np.ndarray:
        """Host rows -> normalised float32 rows (computed on the host)."""
        rows = self._rows(rows)
        out = np.empty(rows.shape, np.float32)
        _lib.check(_lib.lib().bdr_obs_norm_apply(self._h, rows.shape[0], _p(rows), _dtype_code(rows), _p(out)))
        return out

    def apply_device(self, ptr: int, n: int, stride: int, out_ptr: int, out_stride: int, dtype=np.float32) -> None:
        """Rows in HBM (row k at ptr + k * stride bytes, elements of `dtype`) -> float32 rows at out_ptr + k * out_stride: the
        input of `*.sample_device`."""
        code = _lib.BDR_DTYPE_F32 if np.dtype(dtype) == np.float32 else _lib.BDR_DTYPE_F64
        _lib.check(_lib.lib().bdr_obs_norm_apply_device(self._h, n, C.c_void_p(ptr), stride, code, C.c_void_p(out_ptr), out_stride))


def create_replay_buffer(episodes: Iterable, normalizer: Optional[ObsNormalizer] = None, episode_indices: Optional[Sequence[int]] = None,
                         obs_key: Optional[str] = None, device: int = 0, act_dtype=np.float32) -> SimpleReplayBuffer:
    """MinariDataset::create_replay_buffer (dataset.rs:64-109): capacity = the number of transitions, seed 0, no PER, episodes pushed
    in order (boundaries between them are not kept), then num_terminated_flags / num_truncated_flags / sum_rewards are logged.
    `episode_indices` keeps the episodes at those positions of `episodes` (None: all)."""
    episodes = list(episodes)
    if episode_indices is not None:
        keep = set(int(i) for i in episode_indices)
        episodes = [ep for k, ep in enumerate(episodes) if k in keep]
    if not episodes:
        raise ValueError("no episodes")
    num_transitions = sum(int(np.asarray(_field(ep, "rewards")).size) for ep in episodes)
    first_obs, first_act = episode_arrays(episodes[0], obs_key)[:2]
    act_shape = tuple(np.asarray(first_act).shape[1:]) or (1,)
    rb = SimpleReplayBuffer(SimpleReplayBufferConfig(capacity=num_transitions, seed=0, per_config=None), (first_obs.shape[1],), np.float32,
                            act_shape=act_shape, act_dtype=act_dtype, device=device)
    for ep in episodes:
        obs, act, rew, term, trunc = episode_arrays(ep, obs_key)
        rb.push_episode(obs, act, rew, term, trunc, normalizer)
    s = rb.summary()
    log.info("In replay buffer:")
    log.info("%d transitions", num_transitions)
    log.info("%d terminated flags", s["num_terminated_flags"])
    log.info("%d truncated flags", s["num_truncated_flags"])
    log.info("%s reward sum", s["sum_rewards"])
    return rb
