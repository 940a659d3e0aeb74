"""Time to turn a pen-sized episode dataset (examples/d4rl/*_pen: 45 float64 observation columns, 24 f32 action columns) into a
normalised replay ring in HBM, two ways in one process, alternating:

  (a) numpy: statistics over the f32-rounded rows, (x32 - mean) / std, obs / next_obs materialised on the host, one `push`
      - the only route without `push_episode`;
  (b) `ObsNormalizer.from_episodes` + one `push_episode` per episode.

Each repetition ends with a read of the last ring row (a device synchronise).  The two rings are compared once (bit identity of
rows, cursor, size; mean / std within 1 f32 ulp).  Prints ONE JSON line: medians, min / max of the repetitions, and (b) split
into its statistics and push phases.

  python tools/bench_dataset_load.py --transitions 500000 --episode-len 100 --reps 5 [--route a|b|both]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, A = 45, 24


def make_dataset(n_transitions, T, seed=0):
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.01, 10.0, D)
    shift = rng.uniform(-100.0, 100.0, D)
    eps = []
    for _ in range(n_transitions // T):
        term = np.zeros(T, np.int8)
        term[-1] = 1
        eps.append(SimpleNamespace(observations=rng.standard_normal((T + 1, D)) * scale + shift,
                                   actions=rng.uniform(-1, 1, (T, A)).astype(np.float32), rewards=rng.standard_normal(T).astype(np.float32),
                                   terminations=term, truncations=np.zeros(T, np.int8)))
    return eps


def ring(B, n):
    return B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=n, seed=0), (D,), np.float32, act_shape=(A,), act_dtype=np.float32)


def route_a(B, eps, n):
    t0 = time.perf_counter()
    rows = np.concatenate([e.observations.astype(np.float32) for e in eps])            # [n + E][D], f32-rounded
    keep = np.ones(rows.shape[0], bool)
    keep[np.cumsum([e.observations.shape[0] for e in eps]) - 1] = False               # an episode's last row does not count
    first = np.ones(rows.shape[0], bool)
    first[np.cumsum([0] + [e.observations.shape[0] for e in eps[:-1]])] = False        # ... and its first row is nobody's next_obs
    counted = rows[keep].astype(np.float64)
    mean = counted.mean(axis=0).astype(np.float32)
    std = counted.std(axis=0, ddof=1).astype(np.float32)
    t1 = time.perf_counter()
    z = (rows - mean) / std
    obs, nxt = z[keep], z[first]
    cat = lambda k: np.concatenate([getattr(e, k) for e in eps])
    rb = ring(B, n)
    rb.push(obs, cat("actions"), nxt, cat("rewards"), cat("terminations"), cat("truncations"))
    rb.read_rows(n - 1, 1)
    t2 = time.perf_counter()
    return rb, (mean, std), (t2 - t0, t1 - t0, t2 - t1)


def route_b(B, eps, n):
    t0 = time.perf_counter()
    nz = B.ObsNormalizer.from_episodes(eps)
    t1 = time.perf_counter()
    rb = ring(B, n)
    for e in eps:
        rb.push_episode(e.observations, e.actions, e.rewards, e.terminations, e.truncations, nz)
    rb.read_rows(n - 1, 1)
    t2 = time.perf_counter()
    stats = (nz.mean, nz.std)
    nz.close()
    return rb, stats, (t2 - t0, t1 - t0, t2 - t1)


def ulps(a, b):
    o = lambda x: np.where(x.view(np.int32) < 0, -(x.view(np.int32).astype(np.int64) & 0x7FFFFFFF), x.view(np.int32).astype(np.int64))
    return int(np.abs(o(np.asarray(a, np.float32)) - o(np.asarray(b, np.float32))).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transitions", type=int, default=500_000)
    ap.add_argument("--episode-len", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route", choices=("a", "b", "both"), default="both")
    args = ap.parse_args()
    import border_amd as B
    assert B.device_count() >= 1, "needs an MI355X"
    eps = make_dataset(args.transitions, args.episode_len)
    n = sum(len(e.rewards) for e in eps)
    routes = {"a": route_a, "b": route_b}
    names = ["a", "b"] if args.route == "both" else [args.route]
    out = {"transitions": n, "episodes": len(eps), "obs_columns": D, "obs_dtype": "float64", "act_columns": A, "reps": args.reps}
    if args.route == "both":   # untimed: warm-up of both routes, and the comparison of what they build
        (ra, sa, _), (rb_, sb, _) = route_a(B, eps, n), route_b(B, eps, n)
        out["stats_max_ulp"] = max(ulps(sa[0], sb[0]), ulps(sa[1], sb[1]))
        same_stats = out["stats_max_ulp"] == 0
        rows_equal = all(x.tobytes() == y.tobytes() for x, y in zip(ra.read_rows(0, 4096), rb_.read_rows(0, 4096)))
        out["rings_identical_first_4096_rows"] = bool(rows_equal) if same_stats else None   # (rows can only be compared under equal statistics)
        assert ra.head == rb_.head and ra.len() == rb_.len()
        ra.close(); rb_.close()
    else:
        routes[names[0]](B, eps, n)[0].close()
    times = {k: [] for k in names}
    for _ in range(args.reps):
        for k in names:
            rb, _, t = routes[k](B, eps, n)
            rb.close()
            times[k].append(t)
    for k in names:
        t = np.array(times[k])
        out[k] = {"median_s": float(np.median(t[:, 0])), "min_s": float(t[:, 0].min()), "max_s": float(t[:, 0].max()),
                  "statistics_median_s": float(np.median(t[:, 1])), "normalise_and_push_median_s": float(np.median(t[:, 2])),
                  "all_s": [round(float(x), 4) for x in t[:, 0]]}
    if args.route == "both":
        out["speedup_median"] = out["a"]["median_s"] / out["b"]["median_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
