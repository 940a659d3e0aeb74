"""What a push into the single-frame store costs an actor whose frame stacks live in HBM (bdr_atari_prep), per call, n = 1 and n = 256:
  (a) today's only way: copy the two stacks of every transition to the host (2 x n x 28 224 bytes, two bdr_atari_prep_obs reads:
      the library has no read of the previous stacks, so the current ones are read twice - the same bytes over the same path)
      and bdr_replay_push them - the host compares the rows and sends the new frames back;
  (b) bdr_replay_push_device_frames: the rows are compared and the new frames copied inside HBM;
  (c) bdr_replay_push_device into a plain ring (no sharing: 8x the HBM), for scale.
One process; every iteration steps the preprocessor (not timed: new frames shift into the stacks, so obs continues the previous
next_obs as in a running environment), then times the three calls one after the other on the same transition, each into its own
buffer.  Every call ends synchronised (it returns when the caller's rows may be reused).  Medians over --calls iterations after
--warmup.  Prints one JSON line and writes it to --out.

    python tools/bench_push_frames.py [--calls 1000] [--warmup 50] [--out profiles/bench_push_frames.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import border_amd as B

ROW = 4 * 84 * 84
SHAPE = (4, 1, 84, 84)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=50)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_push_frames.json"))
args = ap.parse_args()
if B.device_count() == 0:
    sys.exit("bench_push_frames: no GPU visible (there is no CPU path to time)")

rng = np.random.default_rng(0)
result = {"bench": "push_frames", "calls": args.calls, "warmup": args.warmup, "unit": "us per call, median"}
for n in (1, 256):
    cap = 20_000
    prep = B.AtariPreprocessor(n)
    ixs = np.arange(n)
    pool = [rng.integers(0, 256, (n, 210, 160, 3), dtype=np.uint8) for _ in range(4)]
    prep.reset_device(ixs, pool[0])
    mk = lambda fs: B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=42, frame_stack=fs, frame_capacity=8 * cap + 64 if fs else 0), SHAPE, "uint8")
    rb_a, rb_b, rb_c = mk(4), mk(4), mk(0)
    act = np.zeros((n, 1), np.int64); rew = np.zeros(n, np.float32); fl = np.zeros(n, np.int8)
    last = {"obs": prep.obs(ixs)}     # the bytes of the previous stacks: what the first of the two reads would return

    def call_a():
        prep.obs(ixs)
        nobs = prep.obs(ixs)
        rb_a.push(last["obs"], act, nobs, rew, fl, fl)
        last["obs"] = nobs

    def call_b():
        rb_b.push_device_frames(prep.device_prev_stacks(), ROW, act, prep.device_stacks(), ROW, rew, fl, fl)

    def call_c():
        rb_c.push_device(prep.device_prev_stacks(), ROW, act, prep.device_stacks(), ROW, rew, fl, fl)

    calls = (("a_host_push_with_d2h", call_a), ("b_push_device_frames", call_b), ("c_push_device_plain_ring", call_c))
    t = {name: [] for name, _ in calls}
    for it in range(args.warmup + args.calls):
        prep.step_device(ixs, pool[it % 4], pool[(it + 1) % 4])
        for name, f in calls:
            t0 = time.perf_counter()
            f()
            dt = time.perf_counter() - t0
            if it >= args.warmup:
                t[name].append(1e6 * dt)
    assert rb_a.frames_used() == rb_b.frames_used() and len(rb_a) == len(rb_b) == len(rb_c)
    result[f"n{n}"] = {name: round(float(np.median(v)), 1) for name, v in t.items()}
    result[f"n{n}"]["p10_p90"] = {name: [round(float(np.percentile(v, 10)), 1), round(float(np.percentile(v, 90)), 1)] for name, v in t.items()}
    result[f"n{n}"]["frames_per_transition"] = round(rb_b.frames_used()[0] / ((args.warmup + args.calls) * n), 3)
    rb_a.close(); rb_b.close(); rb_c.close(); prep.close()

line = json.dumps(result)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(line + "\n")
