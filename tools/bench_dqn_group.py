"""Aggregate member-updates/s of a DqnGroup (one launch per group step, one workgroup per member) against the same P standalone
agents stepped in a loop by Agent::opt, and group.sample against P sample calls - BASELINE config C1 (Mlp[64, 64], batch 32,
ring pre-filled) at P in {1, 8, 64, 256}, both sides in one process.

Protocol: warm-up, one window of K = 300 steps per side, then five legs of 0.3 s per side, the two sides alternating; the figure
is the median of the legs, the spread their min / max.  Writes one JSON document (default profiles/bench_dqn_group.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import border_amd as B  # noqa: E402


def c1(seed):
    return B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.MlpConfig(in_dim=4, units=(64, 64), out_dim=2), opt_config=B.OptimizerConfig.Adam(1e-3)),
                       soft_update_interval=1, batch_size=32, tau=0.01, critic_loss="Mse", device=0, param_seed=seed, train=True)


def ring(seed, rows):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=10000, seed=seed), (4,), np.float32)
    rb.push(*rows)
    return rb


def legs(step, sync, per_step, n_legs, leg_s, chunk):
    """rates (units/s) of n_legs legs of about leg_s seconds: `chunk` steps at a time until the time is up, then a synchronise"""
    out = []
    for _ in range(n_legs):
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < leg_s:
            for _ in range(chunk): step()
            n += chunk
        sync()
        out.append(n * per_step / (time.perf_counter() - t0))
    return out


def measure(a_step, a_sync, b_step, b_sync, per_step, K, n_legs, leg_s):
    """a = the group, b = the sequential loop; alternating legs"""
    for step, sync in ((a_step, a_sync), (b_step, b_sync)):
        for _ in range(50): step()
        sync()
    res = {}
    for name, step, sync in (("group", a_step, a_sync), ("loop", b_step, b_sync)):
        t0 = time.perf_counter()
        for _ in range(K): step()
        sync()
        res[name + "_window"] = K * per_step / (time.perf_counter() - t0)
    la, lb = [], []
    for _ in range(n_legs):
        la += legs(a_step, a_sync, per_step, 1, leg_s, 20)
        lb += legs(b_step, b_sync, per_step, 1, leg_s, 5)
    res["group"] = statistics.median(la); res["group_min_max"] = [min(la), max(la)]
    res["loop"] = statistics.median(lb); res["loop_min_max"] = [min(lb), max(lb)]
    res["ratio"] = res["group"] / res["loop"]
    res["ratio_worst_case"] = min(la) / max(lb)
    res["group_step_us"] = 1e6 * per_step / res["group"]
    return {k: (round(v, 2) if isinstance(v, float) else [round(x, 1) for x in v]) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_dqn_group.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n = 5000
    rows = (rng.standard_normal((n, 4)).astype(np.float32), rng.integers(0, 2, (n, 1)).astype(np.int64),
            rng.standard_normal((n, 4)).astype(np.float32), np.ones(n, np.float32), (rng.random(n) < .1).astype(np.int8), np.zeros(n, np.int8))
    doc = {"bench": "dqn_group", "shape": "Mlp[64,64] in 4 A 2, batch 32, ring 5000 / 10000", "window_steps": args.window, "legs": args.legs,
           "leg_seconds": args.leg_seconds, "unit_opt": "member-updates/s (median of the legs)", "unit_sample": "member-actions/s (median of the legs)",
           "opt": {}, "sample": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.DqnGroup.build([c1(i) for i in range(P)])
        g_rings = [ring(100 + i, rows) for i in range(P)]
        solo = [B.Dqn.build(c1(i)) for i in range(P)]
        s_rings = [ring(100 + i, rows) for i in range(P)]
        obs = np.ascontiguousarray(rows[0][:P])       # one [P, in_dim] array: the group's rows by address arithmetic
        obs1 = [obs[i:i + 1] for i in range(P)]
        g.opt(g_rings)                                # names the buffers; opt() then steps on them again

        def loop_opt():
            for a, r in zip(solo, s_rings): a.opt(r)

        def loop_sync():
            for a in solo: a.sync()

        def loop_sample():
            for a, o in zip(solo, obs1): a.sample(o)

        doc["opt"][str(P)] = measure(g.opt, g.sync, loop_opt, loop_sync, P, args.window, args.legs, args.leg_seconds)
        doc["sample"][str(P)] = measure(lambda: g.sample(obs), lambda: None, loop_sample, lambda: None, P, args.window, args.legs, args.leg_seconds)
        print(P, "opt", doc["opt"][str(P)], flush=True)
        print(P, "sample", doc["sample"][str(P)], flush=True)
        g.close()
        for a in solo: a.close()
        for r in g_rings + s_rings: r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.abspath(args.out)}))


if __name__ == "__main__":
    main()
