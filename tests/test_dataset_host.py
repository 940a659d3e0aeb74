"""The dataset path without a GPU: the numpy restatement of the contract against a case worked by hand, the duck typing of
`create_replay_buffer`'s episode access, the loud failure without a device, and header / _lib.py / ffi.rs agreeing on the new symbols."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from border_amd import _lib, build
from tests import dataset_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bdr_obs_norm_create", "bdr_obs_norm_destroy", "bdr_obs_norm_accumulate", "bdr_obs_norm_finish", "bdr_obs_norm_set",
               "bdr_obs_norm_get", "bdr_obs_norm_apply", "bdr_obs_norm_apply_device", "bdr_replay_push_episode", "bdr_replay_summarize")


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_restatement_against_a_case_worked_by_hand():
    # two episodes, dim 2.  Rows that count: [1, 10], [3, 20] (episode 0, T = 2) and [5, 30] (episode 1, T = 1); the last rows do not.
    e0 = np.array([[1., 10.], [3., 20.], [100., 100.]])
    e1 = np.array([[5., 30.], [7., 7.]])
    mean, std, n = R.statistics([e0, e1])
    assert n == 3 and mean.dtype == np.float32 and std.dtype == np.float32
    assert mean.tolist() == [3.0, 20.0]          # (1 + 3 + 5) / 3, (10 + 20 + 30) / 3
    assert std.tolist() == [2.0, 10.0]           # sqrt((4 + 0 + 4) / 2), sqrt((100 + 0 + 100) / 2)   (ddof = 1)
    obs, nxt = R.episode_transitions(e0, mean, std)
    assert obs.tolist() == [[-1.0, -1.0], [0.0, 0.0]]
    assert nxt.tolist() == [[0.0, 0.0], [48.5, 8.0]]   # (100 - 3) / 2, (100 - 20) / 10
    obs, nxt = R.episode_transitions(e1, mean, std)
    assert obs.tolist() == [[1.0, 1.0]] and nxt.dtype == np.float32
    assert nxt.tolist() == [[2.0, float(np.float32(-1.3))]]   # (7 - 3) / 2; -13 / 10 correctly rounded to f32
    # without statistics: the conversion alone, round to nearest even at the f32 grid
    x = np.array([[1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]])      # ties: to the even neighbour 1.0, to the even neighbour 1 + 2^-22
    assert R.normalize(x).tolist() == [[1.0, 1.0 + 2.0 ** -22]]
    # two roundings, not one: (x32 - m) rounds before the division
    m, s = np.array([1.0], np.float32), np.array([3.0], np.float32)
    z = R.normalize(np.array([[1.0 + 2.0 ** -24 + 2.0 ** -40]]), m, s)   # x32 = 1 + 2^-23, difference 2^-23 exactly
    assert z.tolist() == [[float(np.float32(2.0 ** -23) / np.float32(3.0))]]
    # the reward sum is the left-to-right f32 fold: 1e8 + 1 = 1e8 in f32, so the first 1 is lost and the second survives
    assert R.sum_rewards([1e8, 1.0, -1e8, 1.0]) == np.float32(1.0)
    assert R.sum_rewards([1.0, 1.0, 1e8, -1e8]) == np.float32(0.0)
    assert R.ulp_distance(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))) == 1
    assert R.ulp_distance(np.float32(-0.0), np.float32(0.0)) == 0


def test_the_fixed_test_set_is_what_the_gpu_tests_assume():
    eps = R.fixed_test_set()
    assert len(eps) == 40 and all(1 <= len(e.rewards) < 200 and e.observations.shape == (len(e.rewards) + 1, 45) for e in eps)
    assert eps[0].observations.dtype == np.float64
    mean, std, n = R.statistics([e.observations for e in eps])
    assert n == sum(len(e.rewards) for e in eps)
    assert abs(mean[3] - 1000) < 0.01 and abs(std[3] - 0.01) < 2e-3 and abs(mean[7] + 3e4) < 1 and abs(std[9] - 1e-3) < 2e-4
    obs, act, nxt, rew, term, trunc = R.pushed_arrays(eps, mean, std)
    assert obs.shape == (n, 45) and nxt.shape == (n, 45) and act.shape == (n, 24) and obs.dtype == np.float32
    assert np.isfinite(obs).all() and np.isfinite(nxt).all() and max(np.abs(obs).max(), np.abs(nxt).max()) < 5
    # a streaming sum / sum of squares in float64 is NOT good enough for column 3 (which is why the library merges block moments)
    rows = np.concatenate([R.to_f32(e.observations)[:-1] for e in eps]).astype(np.float64)
    naive = np.sqrt((np.cumsum(rows[:, 3] ** 2)[-1] - np.cumsum(rows[:, 3])[-1] ** 2 / n) / (n - 1)).astype(np.float32)
    assert R.ulp_distance(naive, std[3]) > 1
    # the sequential reward sum differs from numpy's pairwise one on these rewards: the order is observable
    assert R.sum_rewards(rew) != np.sum(rew)
    assert 0 < term.sum() < 40 and trunc.sum() > 0


class _Ep:
    def __init__(self, e):
        self.observations, self.actions, self.rewards = e.observations, e.actions, e.rewards
        self.terminations, self.truncations = e.terminations, e.truncations


def test_episode_access_is_duck_typed():
    from border_amd import dataset
    e = R.make_episode(np.random.default_rng(1), 5)
    as_obj, as_dict = _Ep(e), {k: getattr(e, k) for k in dataset.EPISODE_FIELDS}
    nested = dict(as_dict, observations={"observation": e.observations, "desired_goal": np.zeros((6, 2))})
    for ep, key in ((as_obj, None), (as_dict, None), (nested, "observation"), (SimpleNamespace(**nested), "observation")):
        obs, act, rew, term, trunc = dataset.episode_arrays(ep, key)
        assert obs.dtype == np.float64 and (obs == e.observations).all() and (act == e.actions).all() and (rew == e.rewards).all()
        assert (term == e.terminations).all() and (trunc == e.truncations).all()
    f32 = dict(as_dict, observations=e.observations.astype(np.float32))
    assert dataset.episode_arrays(f32)[0].dtype == np.float32
    ints = dict(as_dict, observations=np.arange(12).reshape(6, 2))
    assert dataset.episode_arrays(ints)[0].dtype == np.float64
    with pytest.raises(ValueError):
        dataset.episode_arrays(dict(as_dict, observations=e.observations[:-1]))
    import sys
    assert "minari" not in sys.modules


def test_no_device_fails_loudly(L):
    if _lib.device_count() > 0:
        h = C.c_void_p()
        assert L.bdr_obs_norm_create(0, 0, C.byref(h)) == 1   # dim 0: BDR_ERR_INVALID, with or without a device
        return
    h = C.c_void_p()
    assert L.bdr_obs_norm_create(0, 45, C.byref(h)) == 2      # BDR_ERR_NO_DEVICE
    assert b"no HIP device" in L.bdr_last_error()
    from border_amd import ObsNormalizer, create_replay_buffer
    with pytest.raises(_lib.BdrError):
        ObsNormalizer(45)
    with pytest.raises(_lib.BdrError):
        create_replay_buffer([R.make_episode(np.random.default_rng(1), 5)])


def test_header_loader_and_rust_shim_agree_on_the_new_symbols(L):
    hdr = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"BDR_API int32_t {name}\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
        assert re.search(rf"pub fn {name}\(", ffi), name
    # argument counts: header == ctypes == ffi.rs
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        n_hdr = len(re.search(rf"{name}\((.*?)\)\s*;", flat, flags=re.S).group(1).split(","))
        n_rs = len([p for p in re.search(rf"pub fn {name}\((.*?)\)\s*->", ffi, flags=re.S).group(1).split(",") if p.strip()])
        assert n_hdr == len(getattr(L, name).argtypes) == n_rs, (name, n_hdr, n_rs)
    assert re.search(r"#define BDR_DTYPE_F32 0\b", hdr) and re.search(r"#define BDR_DTYPE_F64 1\b", hdr)
    assert (_lib.BDR_DTYPE_F32, _lib.BDR_DTYPE_F64) == (0, 1)
    assert "pub const BDR_DTYPE_F32: i32 = 0;" in ffi and "pub const BDR_DTYPE_F64: i32 = 1;" in ffi
    assert "pub enum bdr_obs_norm {}" in ffi        # the opaque handle: no #[repr(C)] struct (tests/test_rust_shim_layout.py pins that set)
    assert C.sizeof(_lib.ReplaySummaryC) == 24
    assert [f for f, _ in _lib.ReplaySummaryC._fields_] == ["n_terminated", "n_truncated", "sum_rewards", "reserved"]
    crate = os.path.join(ROOT, "rust", "border-amd-agent", "src")
    assert re.search(r"^pub mod dataset;", open(os.path.join(crate, "lib.rs")).read(), re.M)
    ds = open(os.path.join(crate, "dataset.rs")).read()
    assert "impl Drop for AmdObsNorm" in ds and "bdr_obs_norm_destroy" in ds
    rb = open(os.path.join(crate, "replay.rs")).read()
    for s in ("pub fn push_episode", "pub fn summary", "pub fn whole_actions"):
        assert s in rb, s
