"""Aggregate member-updates/s of an IqlGroup (3 (Lq + Lv) + 2 Lp + 8 = 40 launches per round whatever P is) against a loop of Agent::opt
(bdr_agent_opt) over the same P agents standalone, in one process, at the pen shape: obs 45, act 24, value, critic and actor
Mlp[256, 256, 256], two critics, B = 256, Adam - P in {1, 8, 64}.  The data of both sides are VIEWS of one ring of 100 000 rows
(SimpleReplayBuffer.view): P index streams over one copy of the rows.

Protocol (tools/bench_dqn_group.py --wide, tools/bench_bc_group.py): warm-up, one window of K = 300 rounds per side, then five legs of
0.3 s per side, the two sides alternating; the figure is the median of the legs, the spread their min / max.  The bar: at P = 8 the
group's worst leg lies above the loop's best leg; P = 1 (the group's cost against the agent alone) and P = 64 are reported without
one.  Writes one JSON document (default profiles/bench_iql_group.json)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_amd as B  # noqa: E402
from bench_dqn_group import measure  # noqa: E402
from border_amd.iql import CandleMlpConfig, GaussianActorConfig, IqlConfig, MultiCriticConfig, ValueConfig  # noqa: E402

OBS, ACT, UNITS, BATCH, ROWS = 45, 24, (256, 256, 256), 256, 100_000


def config(i):
    """a sweep over expectile, temperature and seed"""
    opt = lambda: B.OptimizerConfig.Adam(3e-4)
    return IqlConfig(obs_dim=OBS, act_dim=ACT, value_config=ValueConfig(CandleMlpConfig(UNITS), opt()),
                     critic_config=MultiCriticConfig(2, CandleMlpConfig(UNITS), opt(), 0.005),
                     actor_config=GaussianActorConfig(CandleMlpConfig(UNITS), opt()), tau_iql=0.5 + 0.1 * (i % 5), inv_lambda=(0.5, 3.0, 10.0)[i % 3],
                     batch_size=BATCH, seed=i, device=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_iql_group.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    owner = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=ROWS, seed=1), (OBS,), np.float32, (ACT,), np.float32, device=0)
    for _ in range(ROWS // 10_000):
        n = 10_000
        owner.push(rng.standard_normal((n, OBS)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ACT)).astype(np.float32),
                   rng.standard_normal((n, OBS)).astype(np.float32), rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.01).astype(np.int8),
                   np.zeros(n, np.int8))
    doc = {"bench": "iql_group", "shape": "pen: obs 45, act 24, value / critic / actor Mlp[256,256,256], 2 critics, B 256, Adam; views of one ring of 100000 rows",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-updates/s (median of the legs); loop = bdr_agent_opt of the same P agents standalone, one after the other",
           "bar": "at P = 8: group_min > loop_max", "opt": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.IqlGroup.build([config(i) for i in range(P)])
        solo = [B.Iql.build(config(i)) for i in range(P)]
        gv, sv = [owner.view(100 + i) for i in range(P)], [owner.view(100 + i) for i in range(P)]
        g.opt(gv)   # names the buffers; opt() then goes on with them

        def loop():
            for a, v in zip(solo, sv): a.opt(v)

        def loop_sync():
            for a in solo: a.sync()

        m = measure(g.opt, g.sync, loop, loop_sync, P, args.window, args.legs, args.leg_seconds)
        m["launches_per_round"] = g.launches_per_round
        if P == 8:
            m["bar_met"] = bool(m["group_min_max"][0] > m["loop_min_max"][1])
        doc["opt"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
        for v in gv + sv: v.close()
    owner.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(args.out))


if __name__ == "__main__":
    main()
