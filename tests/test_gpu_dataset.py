"""Episode ingestion and observation normalisation on the MI355X against the numpy restatement (tests/dataset_restatement.py):
`ObsNormalizer` statistics, `push_episode` == `push` of the restatement's arrays (ring bytes, cursor, size, PER tree, batches),
`apply` / `apply_device`, `summary`, an IQL run over both rings, and the refusals.

Bounds.  Statistics: 1 f32 ulp - the float64 accumulation error (about 1e-13 relative on this set) is far below half an f32 ulp, so
the rounded device result is the correctly rounded value or, when the exact value lies within that error of a rounding boundary, its
neighbour; the same holds for the restatement.  Everything else is bit identity: the element contract fixes every rounding.

"A normaliser on another device" needs a second GPU; on a one-GPU box that single refusal is not exercised (the others are)."""
import os
import re

import numpy as np
import pytest

from tests import dataset_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


@pytest.fixture(scope="module")
def eps():
    return R.fixed_test_set()


@pytest.fixture(scope="module")
def stats(eps):
    return R.statistics([e.observations for e in eps])


def _normalizer(B, eps, f32=False):
    nz = B.ObsNormalizer(R.D)
    for e in eps:
        nz.accumulate(R.to_f32(e.observations[:-1]) if f32 else e.observations[:-1])
    return nz.finish()


def _ring(B, capacity, per=False, seed=5):
    cfg = B.SimpleReplayBufferConfig(capacity=capacity, seed=seed, per_config=B.PerConfig() if per else None)
    return B.SimpleReplayBuffer(cfg, (R.D,), np.float32, act_shape=(R.ACT_DIM,), act_dtype=np.float32)


def _push_episodes(rb, eps, nz, f32=False):
    for e in eps:
        rb.push_episode(R.to_f32(e.observations) if f32 else e.observations, e.actions, e.rewards, e.terminations, e.truncations, nz)


def _same_ring(a, b, capacity):
    assert a.head == b.head and a.len() == b.len()
    for x, y in zip(a.read_rows(0, capacity), b.read_rows(0, capacity)):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. statistics
def test_statistics_are_within_one_ulp_of_the_restatement_and_reproducible(B, eps, stats):
    mean, std, n = stats
    a, b = _normalizer(B, eps), _normalizer(B, eps)
    assert a.count == n == b.count
    print("max ulp distance: mean", R.ulp_distance(a.mean, mean).max(), "std", R.ulp_distance(a.std, std).max())
    assert R.ulp_distance(a.mean, mean).max() <= 1
    assert R.ulp_distance(a.std, std).max() <= 1
    assert (_bits(a.mean) == _bits(b.mean)).all() and (_bits(a.std) == _bits(b.std)).all()     # two runs, the same bits
    # from_episodes is the same sequence of rows
    c = B.ObsNormalizer.from_episodes(eps)
    assert (_bits(c.mean) == _bits(a.mean)).all() and (_bits(c.std) == _bits(a.std)).all() and c.count == n
    # float32 input == float64 input holding the same (f32-representable) values
    f32 = _normalizer(B, eps, f32=True)
    wide = B.ObsNormalizer(R.D)
    for e in eps:
        wide.accumulate(R.to_f32(e.observations[:-1]).astype(np.float64))
    wide.finish()
    for nz in (f32, wide):
        assert (_bits(nz.mean) == _bits(a.mean)).all() and (_bits(nz.std) == _bits(a.std)).all()
    # ... and however the rows are cut into calls
    one = B.ObsNormalizer(R.D).accumulate(np.concatenate([e.observations[:-1] for e in eps])).finish()
    assert (_bits(one.mean) == _bits(a.mean)).all() and (_bits(one.std) == _bits(a.std)).all()
    # set / get round trip
    s = B.ObsNormalizer(R.D).set(mean, std)
    assert (_bits(s.mean) == _bits(mean)).all() and (_bits(s.std) == _bits(std)).all() and s.count == 0
    for nz in (a, b, c, f32, wide, one, s):
        nz.close()


# ------------------------------------------------------------------------------------------------ 2. ring identity
@pytest.mark.parametrize("f32", [False, True], ids=["float64", "float32"])
@pytest.mark.parametrize("with_norm", [True, False], ids=["normalised", "converted"])
def test_push_episode_equals_push_of_the_restatements_arrays(B, eps, f32, with_norm):
    nz = _normalizer(B, eps) if with_norm else None
    mean, std = (nz.mean, nz.std) if with_norm else (None, None)
    arrays = R.pushed_arrays(eps, mean, std, f32_input=f32)
    n = arrays[3].shape[0]
    for capacity in (n, n + 17, (n * 3) // 5):              # exactly full, not full, wrapped
        a, b = _ring(B, capacity), _ring(B, capacity)
        _push_episodes(a, eps, nz, f32)
        b.push(*arrays)
        _same_ring(a, b, capacity)
        ba, bb = a.batch(256), b.batch(256)
        for x, y in zip(ba.unpack()[:7], bb.unpack()[:7]):
            assert x.tobytes() == y.tobytes()
        if capacity == n:
            assert (a.whole_actions() == arrays[1]).all()
        a.close(); b.close()
    if nz is not None:
        nz.close()


def _staging_bytes():
    src = open(os.path.join(ROOT, "border_amd", "csrc", "replay.hip")).read()
    m = re.search(r"constexpr uint64_t EPISODE_STAGE_BYTES = (\d+)ull << (\d+);", src)
    return int(m.group(1)) << int(m.group(2))


@pytest.mark.parametrize("f32", [False, True], ids=["float64", "float32"])
def test_a_long_episode_a_one_step_episode_and_a_wrap_inside_a_pass(B, eps, stats, f32):
    mean, std, _ = stats
    rng = np.random.default_rng(11)
    T_long = _staging_bytes() // (R.D * 4) + 1000           # more rows than one staging half holds, for either dtype
    seq = [R.make_episode(rng, 1), R.make_episode(rng, T_long), R.make_episode(rng, 1), eps[0], R.make_episode(rng, 1)]
    arrays = R.pushed_arrays(seq, mean, std, f32_input=f32)
    n = arrays[3].shape[0]
    nz = B.ObsNormalizer(R.D).set(mean, std)
    for capacity in (n, T_long - 777):                        # the long episode alone wraps the smaller ring
        a, b = _ring(B, capacity), _ring(B, capacity)
        _push_episodes(a, seq, nz, f32)
        for lo in range(0, n, 4096):                          # (push stages in small runs; any cut gives the same ring)
            b.push(*[x[lo:lo + 4096] for x in arrays])
        _same_ring(a, b, capacity)
        a.close(); b.close()
    # T == 0 is a no-op
    a = _ring(B, 8)
    a.push_episode(np.zeros((1, R.D)), np.zeros((0, R.ACT_DIM), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int8), np.zeros(0, np.int8), nz)
    assert a.len() == 0 and a.head == 0
    a.close(); nz.close()


# ------------------------------------------------------------------------------------------------ 3. PER
def test_per_priorities_are_those_of_push(B, eps):
    nz = _normalizer(B, eps)
    arrays = R.pushed_arrays(eps, nz.mean, nz.std)
    n = arrays[3].shape[0]
    for capacity in (n, (n * 3) // 5):
        a, b = _ring(B, capacity, per=True), _ring(B, capacity, per=True)
        _push_episodes(a, eps, nz)
        lo = 0
        for e in eps:                                          # set_priority runs once per push: the same cuts on both sides
            T = len(e.rewards)
            b.push(*[x[lo:lo + T] for x in arrays])
            lo += T
        _same_ring(a, b, capacity)
        assert a.per_tree().tobytes() == b.per_tree().tobytes()
        assert a.per_info() == b.per_info()
        ba, bb = a.batch(256), b.batch(256)
        assert (ba.ix_sample == bb.ix_sample).all() and ba.weight.tobytes() == bb.weight.tobytes() and ba.obs.tobytes() == bb.obs.tobytes()
        a.close(); b.close()
    nz.close()


# ------------------------------------------------------------------------------------------------ 4. apply
def test_apply_and_apply_device_give_the_restatements_bits(B, eps, stats):
    import torch
    nz = _normalizer(B, eps)
    mean, std = nz.mean, nz.std
    rows = np.concatenate([e.observations for e in eps[:6]])
    n = rows.shape[0]
    for x in (rows, R.to_f32(rows)):
        want = R.normalize(x, mean, std)
        got = nz.apply(x)
        assert got.dtype == np.float32 and (_bits(got) == _bits(want)).all()
        tdt = torch.float64 if x.dtype == np.float64 else torch.float32
        eb = x.dtype.itemsize
        # dense rows
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.full((n, R.D), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        nz.apply_device(d_in.data_ptr(), n, R.D * eb, d_out.data_ptr(), R.D * 4, dtype=x.dtype)
        assert (_bits(d_out.cpu().numpy()) == _bits(want)).all()
        # strided input and output: rows 64 elements apart, columns 45.. untouched
        wide = torch.zeros((n, 64), dtype=tdt, device="cuda")
        wide[:, :R.D] = d_in
        out_w = torch.full((n, 48), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        nz.apply_device(wide.data_ptr(), n, 64 * eb, out_w.data_ptr(), 48 * 4, dtype=x.dtype)
        o = out_w.cpu().numpy()
        assert (_bits(o[:, :R.D]) == _bits(want)).all() and (o[:, R.D:] == -7.0).all()
    # one row, as at acting time
    assert (_bits(nz.apply(rows[3])) == _bits(R.normalize(rows[3:4], mean, std))).all()
    nz.close()


# ------------------------------------------------------------------------------------------------ 5. summary
def test_summary_counts_and_the_sequential_reward_sum(B, eps):
    arrays = R.pushed_arrays(eps)
    rew, term, trunc = arrays[3], arrays[4], arrays[5]
    rb = B.create_replay_buffer(eps)                           # no normaliser: conversion alone
    assert rb.len() == rew.shape[0] == rb.config.capacity and rb.config.seed == 0 and rb.config.per_config is None
    s = rb.summary()
    want = R.sum_rewards(rew)
    print("sum_rewards", s["sum_rewards"], "sequential", want, "np.sum", np.sum(rew))
    assert s["num_terminated_flags"] == int(term.sum()) and s["num_truncated_flags"] == int(trunc.sum())
    assert want != np.sum(rew)                                 # the order is observable on this input
    assert _bits(s["sum_rewards"]) == _bits(want)
    obs, act, nxt, r, t, u = rb.read_rows(0, rb.len())
    assert obs.tobytes() == arrays[0].tobytes() and nxt.tobytes() == arrays[2].tobytes() and (r == rew).all()
    rb.close()
    # a ring that is not full: rows [0, len) only
    part = _ring(B, rew.shape[0] + 100)
    _push_episodes(part, eps[:7], None)
    k = sum(len(e.rewards) for e in eps[:7])
    s = part.summary()
    assert _bits(s["sum_rewards"]) == _bits(R.sum_rewards(rew[:k]))
    assert (s["num_terminated_flags"], s["num_truncated_flags"]) == (int(term[:k].sum()), int(trunc[:k].sum()))
    part.close()
    # episode_indices and dict episodes with an observation key
    keyed = [{"observations": {"observation": e.observations, "achieved_goal": e.observations[:, :3]}, "actions": e.actions, "rewards": e.rewards,
              "terminations": e.terminations, "truncations": e.truncations} for e in eps]
    sub = B.create_replay_buffer(keyed, episode_indices=[2, 5], obs_key="observation")
    want_sub = R.pushed_arrays([eps[2], eps[5]])
    assert sub.len() == want_sub[3].shape[0]
    assert sub.read_rows(0, sub.len())[0].tobytes() == want_sub[0].tobytes()
    sub.close()


# ------------------------------------------------------------------------------------------------ 6. end to end
def _iql(B):
    mlp = lambda: B.CandleMlpConfig(units=(64, 64))
    cfg = B.IqlConfig(obs_dim=R.D, act_dim=R.ACT_DIM, value_config=B.ValueConfig(value_config=mlp()),
                      critic_config=B.MultiCriticConfig(q_config=mlp()), actor_config=B.GaussianActorConfig(policy_config=mlp()),
                      batch_size=64, train=True, seed=3, device=0)
    return B.Iql.build(cfg)


def test_an_iql_run_over_either_ring_gives_the_same_parameters_and_actions(B, eps):
    import torch
    nz = B.ObsNormalizer.from_episodes(eps)
    by_episode = B.create_replay_buffer(eps, normalizer=nz)
    arrays = R.pushed_arrays(eps, nz.mean, nz.std)
    by_push = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=arrays[3].shape[0], seed=0), (R.D,), np.float32,
                                   act_shape=(R.ACT_DIM,), act_dtype=np.float32)
    by_push.push(*arrays)
    a, b = _iql(B), _iql(B)
    names = ("actor", "value", "critic_0", "critic_1", "critic_tgt_0", "critic_tgt_1")
    before = [a.get_params(m).copy() for m in names]
    for m, p in zip(names, before):
        assert b.get_params(m).tobytes() == p.tobytes(), m
    for _ in range(20):
        a.opt(by_episode); b.opt(by_push)
    a.sync(); b.sync()
    assert a.n_opts == 20 == b.n_opts
    for m, p in zip(names, before):
        assert a.get_params(m).tobytes() == b.get_params(m).tobytes(), m
        assert a.get_params(m).tobytes() != p.tobytes(), m               # the run did train
    # acting on raw environment observations: normalised on the device vs on the host
    raw = eps[3].observations[:9]
    a.eval()
    d_in = torch.from_numpy(raw).cuda()
    d_out = torch.empty((9, R.D), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nz.apply_device(d_in.data_ptr(), 9, R.D * 8, d_out.data_ptr(), R.D * 4, dtype=np.float64)
    on_device = a.sample_device(d_out.data_ptr(), 9, R.D * 4)
    on_host = a.sample(nz.apply(raw))
    assert on_device.tobytes() == on_host.tobytes()
    assert on_host.tobytes() == a.sample(R.normalize(raw, nz.mean, nz.std)).tobytes()
    a.close(); b.close(); by_episode.close(); by_push.close(); nz.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def _refused(B, fn, *needles):
    with pytest.raises(B.BdrError) as ei:
        fn()
    assert ei.value.code == 1, ei.value                       # BDR_ERR_INVALID
    msg = str(ei.value)
    assert len(msg) > len("border_amd error 1: ") and all(s in msg for s in needles), msg


def test_refusals(B, eps, stats):
    mean, std, _ = stats
    e = eps[0]
    args = (e.actions, e.rewards, e.terminations, e.truncations)
    nz = B.ObsNormalizer(R.D).set(mean, std)
    # a normaliser of another dim than the ring's rows
    nz44 = B.ObsNormalizer(44).set(mean[:44], std[:44])
    rb = _ring(B, 64)
    _refused(B, lambda: rb.push_episode(e.observations, *args, nz44), "dim")
    # observation rows of another dim than the ring's
    _refused(B, lambda: rb.push_episode(e.observations[:, :44], *args, None), "dim")
    narrow = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64), (44,), np.float32, act_shape=(R.ACT_DIM,), act_dtype=np.float32)
    _refused(B, lambda: narrow.push_episode(e.observations[:, :44], *args, nz), "dim")
    assert rb.len() == 0 and narrow.len() == 0
    narrow.close()
    # a normaliser on another device
    if B.device_count() >= 2:
        other = B.ObsNormalizer(R.D, device=1).set(mean, std)
        _refused(B, lambda: rb.push_episode(e.observations, *args, other), "device")
        other.close()
    # a normaliser without statistics
    _refused(B, lambda: rb.push_episode(e.observations, *args, B.ObsNormalizer(R.D)), "statistics")
    rb.close()
    # a single-frame (frame_stack) ring
    fs = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, frame_stack=4), (4, 4), np.float32, act_shape=(R.ACT_DIM,), act_dtype=np.float32)
    nz16 = B.ObsNormalizer(16).set(mean[:16], std[:16])
    _refused(B, lambda: fs.push_episode(e.observations[:, :16], *args, nz16), "frame_stack")
    fs.close(); nz16.close()
    # finish with a constant column names the column
    const = B.ObsNormalizer(R.D)
    rows = e.observations[:-1].copy()
    rows[:, 12] = 2.5
    rows[:, 30] = -1.0
    const.accumulate(rows)
    _refused(B, const.finish, "column 12")
    # finish with fewer than two rows
    one = B.ObsNormalizer(R.D).accumulate(e.observations[:1])
    _refused(B, one.finish, "at least 2")
    _refused(B, B.ObsNormalizer(R.D).finish, "at least 2")
    # accumulate after finish, and after set
    done = B.ObsNormalizer(R.D).accumulate(e.observations[:-1]).finish()
    _refused(B, lambda: done.accumulate(e.observations[:-1]), "after finish")
    _refused(B, lambda: nz.accumulate(e.observations[:-1]), "after finish")
    # statistics that cannot normalise
    bad = std.copy()
    bad[5] = 0.0
    _refused(B, lambda: B.ObsNormalizer(R.D).set(mean, bad), "column 5")
    # statistics asked for before there are any
    _refused(B, lambda: B.ObsNormalizer(R.D).mean, "no statistics")
    for h in (nz, nz44, const, one, done):
        h.close()
