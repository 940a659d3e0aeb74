"""numpy restatement of the dataset contract (include/border_amd.h, "Episode datasets and observation normalisation"):

  element      x32 = x.astype(float32)   (float64 -> f32, round to nearest even: Rust's `as f32`)
               z   = (x32 - mean32) / std32   in float32: two separately rounded operations (ndarray's `(&obs - &mean) / &std`,
                                              border-minari/src/d4rl/pen/candle.rs:71-74)
  statistics   over the first T rows of every episode (the reference drops the last row, pen/candle.rs:56, 146-152), in float64
               over the f32-rounded rows: mean = sum / n, std = sqrt(sum (x - mean)^2 / (n - 1)), each rounded to f32 once
  episode      obs = N(observations[0:T]), next_obs = N(observations[1:T+1])   (pen/candle.rs:104-124, 146-161)
  sum_rewards  the left-to-right f32 fold (`Iterator::sum`, border-core/src/generic_replay_buffer/base.rs:265)

and the fixed test set of tests/test_gpu_dataset.py."""
from types import SimpleNamespace

import numpy as np


def to_f32(x):
    return np.asarray(x).astype(np.float32)


def statistics(episode_observations):
    """(mean32, std32, n) over observations[:-1] of every episode."""
    rows = np.concatenate([to_f32(o)[:-1] for o in episode_observations], axis=0).astype(np.float64)
    n = rows.shape[0]
    mean = rows.sum(axis=0) / n
    std = np.sqrt(((rows - mean) ** 2).sum(axis=0) / (n - 1))
    return mean.astype(np.float32), std.astype(np.float32), n


def normalize(x, mean32=None, std32=None):
    x32 = to_f32(x)
    if mean32 is None:
        return x32
    d = x32 - np.asarray(mean32, np.float32)       # float32 - float32 -> float32, rounded
    z = d / np.asarray(std32, np.float32)           # float32 / float32 -> float32, correctly rounded
    assert z.dtype == np.float32
    return z


def episode_transitions(observations, mean32=None, std32=None):
    """(obs, next_obs) of one episode: rows 0..T and 1..T+1."""
    z = normalize(observations, mean32, std32)
    return z[:-1], z[1:]


def sum_rewards(rewards):
    s = np.float32(0.0)
    for r in np.asarray(rewards, np.float32).reshape(-1):
        s = np.float32(s + r)
    return s


def f32_ordinal(a):
    """float32 -> integers that are monotone in the value: |ordinal(a) - ordinal(b)| is the distance in ulps."""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return np.abs(f32_ordinal(a) - f32_ordinal(b))


D, ACT_DIM, N_EPISODES = 45, 24, 40


def make_episode(rng, T, act_dim=ACT_DIM):
    obs = rng.standard_normal((T + 1, D))
    obs[:, 3] = 1000.0 + 0.01 * obs[:, 3]      # a mean far larger than the spread
    obs[:, 7] = -3e4 + 2.0 * obs[:, 7]
    obs[:, 9] *= 1e-3
    term = np.zeros(T, np.int8)
    trunc = (rng.random(T) < 0.02).astype(np.int8)
    if rng.random() < 0.5:
        term[-1] = 1
    else:
        trunc[-1] = 1
    return SimpleNamespace(observations=obs, actions=rng.uniform(-1, 1, (T, act_dim)).astype(np.float32),
                           rewards=rng.standard_normal(T).astype(np.float32), terminations=term, truncations=trunc)


def fixed_test_set():
    """np.random.default_rng(7), 40 episodes, T ~ integers(1, 200), D = 45, float64 standard normal; column 3 = 1000 + 0.01 N,
    column 7 = -3e4 + 2 N, column 9 scaled by 1e-3."""
    rng = np.random.default_rng(7)
    Ts = rng.integers(1, 200, size=N_EPISODES)
    return [make_episode(rng, int(T)) for T in Ts]


def pushed_arrays(episodes, mean32=None, std32=None, f32_input=False):
    """What bdr_replay_push would be given for the whole set: (obs, act, next_obs, reward, term, trunc), concatenated."""
    o, x = [], []
    for ep in episodes:
        raw = to_f32(ep.observations) if f32_input else ep.observations
        a, b = episode_transitions(raw, mean32, std32)
        o.append(a); x.append(b)
    cat = lambda k: np.concatenate([np.asarray(getattr(ep, k)) for ep in episodes], axis=0)
    return (np.concatenate(o), cat("actions").astype(np.float32), np.concatenate(x), cat("rewards").astype(np.float32),
            cat("terminations").astype(np.int8), cat("truncations").astype(np.int8))
