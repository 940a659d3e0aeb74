"""Aggregate member-updates/s of a BcGroup (2L + 2 launches per round whatever P is) against a loop of Agent::opt over the same P agents
standalone, in one process, at the bc_pen shape: obs 45, act 24, Mlp[256, 256] with a Tanh output, B = 256, AdamW, the default kernel
form (the MFMA head) - P in {1, 8, 64}.  The data of both sides are VIEWS of one ring of 100 000 rows (SimpleReplayBuffer.view): P index
streams over one copy of the rows.

Protocol (tools/bench_dqn_group.py --wide): warm-up, one window of K = 300 rounds per side, then five legs of 0.3 s per side, the two
sides alternating; the figure is the median of the legs, the spread their min / max.  The bar: at P = 8 the group's worst leg lies
above the loop's best leg; P = 1 and P = 64 are reported without one.  Also reported: us per group round, and the HBM held by the
rows of P views against P rings of their own.  Writes one JSON document (default profiles/bench_bc_group.json)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_amd as B  # noqa: E402
from bench_dqn_group import measure  # noqa: E402

OBS, ACT, UNITS, BATCH, ROWS = 45, 24, (256, 256), 256, 100_000


def config(i):
    opt = B.OptimizerConfig.AdamW(1e-3 * (1 + 0.01 * i))
    return B.BcConfig(obs_dim=OBS, act_dim=ACT, policy_model_config=B.BcModelConfig(B.CandleMlpConfig(UNITS, "Tanh"), opt), batch_size=BATCH,
                      action_type="Continuous", device=0, seed=i)


def ring_bytes(capacity):
    """capacity x record stride (include/border_amd.h: obs | next_obs | act | reward, flags; 16-byte aligned sections)"""
    up = lambda x, a: (x + a - 1) // a * a
    next_off = up(OBS * 4, 16)
    act_off = up(next_off + OBS * 4, 16)
    raw = up(act_off + ACT * 4, 8) + 8
    return capacity * up(raw, 128 if raw >= 1024 else 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_bc_group.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    owner = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=ROWS, seed=1), (OBS,), np.float32, (ACT,), np.float32, device=0)
    for _ in range(ROWS // 10_000):
        n = 10_000
        owner.push(rng.standard_normal((n, OBS)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ACT)).astype(np.float32),
                   rng.standard_normal((n, OBS)).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.int8), np.zeros(n, np.int8))
    doc = {"bench": "bc_group", "shape": "bc_pen: obs 45, act 24, Mlp[256,256] Tanh, B 256, AdamW, default kernel form; views of one ring of 100000 rows",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-updates/s (median of the legs); loop = bdr_agent_opt of the same P agents standalone, one after the other",
           "bar": "at P = 8: group_min > loop_max", "opt": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.BcGroup.build([config(i) for i in range(P)])
        solo = [B.Bc.build(config(i)) for i in range(P)]
        gv, sv = [owner.view(100 + i) for i in range(P)], [owner.view(100 + i) for i in range(P)]
        g.opt(gv)   # names the buffers; opt() then goes on with them

        def loop():
            for a, v in zip(solo, sv): a.opt(v)

        def loop_sync():
            for a in solo: a.sync()

        m = measure(g.opt, g.sync, loop, loop_sync, P, args.window, args.legs, args.leg_seconds)
        m["launches_per_round"] = g.launches_per_round
        m["hbm_rows_P_views_MB"] = round(ring_bytes(ROWS) / 1e6, 1)
        m["hbm_rows_P_rings_MB"] = round(P * ring_bytes(ROWS) / 1e6, 1)
        if P == 8:
            m["bar_met"] = bool(m["group_min_max"][0] > m["loop_min_max"][1])
        doc["opt"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
        for v in gv + sv: v.close()
    owner.close()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(args.out))


if __name__ == "__main__":
    main()
