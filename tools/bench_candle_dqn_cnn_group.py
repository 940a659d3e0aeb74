"""Aggregate member-updates/s of a CandleDqnCnnGroup (17 launches per round whatever P is) against a loop of Agent::opt
(bdr_agent_opt) over the same P agents standalone, in one process, at the dqn_atari shape: n_stack 4, 6 actions, B = 32, AdamW, Mse -
P in {1, 8, 32}.  The data of both sides are VIEWS of one u8 ring (SimpleReplayBuffer.view): P index streams over one copy of the rows.

Protocol (tools/bench_candle_dqn_group.py): warm-up, one window of K rounds per side, then five legs of 0.3 s per side, the two sides
alternating, a synchronise per leg; the figure is the median of the legs, the spread their min / max.  The bar, at P = 8 and P = 32:
the group's worst leg is not below the loop's best leg; P = 1 (the cost of a group of one against the agent alone) is reported without
one.  Writes one JSON document (default profiles/bench_candle_dqn_cnn_group.json).

--act    ONE group acting call (CandleDqnCnnGroup.sample: two launches whatever P is) of one host frame stack per member in eval
mode against a loop of the same P agents' own sample() on the image act path, their faster path; member-actions/s, the same protocol
and bar.  Writes profiles/bench_candle_dqn_cnn_group_act.json."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_amd as B  # noqa: E402
from bench_dqn_group import measure  # noqa: E402

N_STACK, ACTIONS, BATCH, ROWS = 4, 6, 32, 4096
ROW = 84 * 84 * N_STACK
SHAPE = "dqn_atari: n_stack 4, 6 actions, B 32, AdamW, Mse"


def config(i):
    """a sweep over seed, learning rate, discount and the soft-update interval"""
    return B.CandleDqnConfig(q_config=B.AtariCnnConfig(n_stack=N_STACK, out_dim=ACTIONS),
                             model_config=B.CandleDqnModelConfig(opt_config=B.OptimizerConfig.AdamW((1e-4, 3e-5)[i % 2])),
                             soft_update_interval=(1, 2, 4)[i % 3], batch_size=BATCH, discount_factor=(0.99, 0.98)[i % 2], tau=0.005, critic_loss="Mse",
                             seed=i, device=0)


def act(args):
    rng = np.random.default_rng(0)
    doc = {"bench": "candle_dqn_cnn_group_act", "shape": SHAPE + "; one host frame stack per member, eval mode", "window_steps": args.window, "legs": args.legs,
           "leg_seconds": args.leg_seconds,
           "unit": "member-actions/s (median of the legs); loop = sample() of the same P agents standalone on the image act path, one after the other",
           "bar": "at P = 8 and P = 32: group_min >= loop_max", "act": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.CandleDqnCnnGroup.build([config(i) for i in range(P)])
        solo = [B.CandleDqn.build(config(i)) for i in range(P)]
        for a in solo: a.set_act_path("image")
        rows = [rng.integers(0, 256, (1, ROW), dtype=np.uint8) for _ in range(P)]

        def loop():
            for a, r in zip(solo, rows): a.sample(r)

        m = measure(lambda: g.sample(rows), g.sync, loop, lambda: None, P, args.window, args.legs, args.leg_seconds)   # (both sides' calls are synchronous)
        if P > 1:
            m["bar_met"] = bool(m["group_min_max"][0] >= m["loop_min_max"][1])
        doc["act"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--act", action="store_true")
    ap.add_argument("--sizes", default="1,8,32")
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                        "bench_candle_dqn_cnn_group_act.json" if args.act else "bench_candle_dqn_cnn_group.json")
    if args.act:
        return write(args, act(args))
    rng = np.random.default_rng(0)
    owner = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=ROWS, seed=1), (ROW,), np.uint8, (1,), np.int64, device=0)
    for _ in range(ROWS // 512):
        n = 512
        owner.push(rng.integers(0, 256, (n, ROW), dtype=np.uint8), rng.integers(0, ACTIONS, (n, 1)).astype(np.int64), rng.integers(0, 256, (n, ROW), dtype=np.uint8),
                   rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))
    doc = {"bench": "candle_dqn_cnn_group", "shape": SHAPE + f"; views of one u8 ring of {ROWS} rows",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-updates/s (median of the legs); loop = bdr_agent_opt of the same P agents standalone, one after the other",
           "bar": "at P = 8 and P = 32: group_min >= loop_max", "opt": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.CandleDqnCnnGroup.build([config(i) for i in range(P)])
        solo = [B.CandleDqn.build(config(i)) for i in range(P)]
        gv, sv = [owner.view(100 + i) for i in range(P)], [owner.view(100 + i) for i in range(P)]
        g.opt(gv)   # names the buffers; opt() then goes on with them

        def loop():
            for a, v in zip(solo, sv): a.opt(v)

        def loop_sync():
            for a in solo: a.sync()

        m = measure(g.opt, g.sync, loop, loop_sync, P, args.window, args.legs, args.leg_seconds)
        if P > 1:
            m["bar_met"] = bool(m["group_min_max"][0] >= m["loop_min_max"][1])
        m["launches_per_round"] = g.launches_per_round
        doc["opt"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
        for v in gv + sv: v.close()
    owner.close()
    write(args, doc)


def write(args, doc):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(args.out))


if __name__ == "__main__":
    main()
