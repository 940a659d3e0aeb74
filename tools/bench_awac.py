"""AWAC update rate at the pen shape of examples/d4rl/awac_pen (obs 45, act 24, [256, 256, 256] for actor and twin critics, B = 256):
Agent::opt over an HBM replay ring holding an offline dataset, in train mode (act_ and next_act drawn from the device stream, as
under Trainer, which calls agent.train()).  Prints ONE JSON line.

  W untimed updates; K timed updates (device-synchronised wall clock); a steady leg of >= 0.3 s repeated `--legs` times (the spread);
  launches per update from the agent's profile brackets (bdr_agent_profile_*); algorithmic GFLOP per update and the share of the FP32
  MFMA peak; the float32 autograd restatement's rate on 16 CPU threads, for context.

  python tools/bench_awac.py --steps 200 --warmup 20
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X: v_mfma_f32_32x32x2_f32, dense (bench.py)
O, A, UNITS, NC, BSZ = 45, 24, (256, 256, 256), 2, 256


def mlp_flops(in_dim, units, out_dim, bsz):
    """(forward, weight-gradient, input-gradient without layer 0) multiply-add FLOPs of one pass"""
    dims = [in_dim] + list(units) + [out_dim]
    mac = [dims[k] * dims[k + 1] for k in range(len(dims) - 1)]
    f = 2 * bsz * sum(mac)
    return f, f, f - 2 * bsz * mac[0]


def update_gflop():
    qf, qw, qx = mlp_flops(O + A, UNITS, 1, BSZ)
    pf, pw, px = mlp_flops(O, UNITS, A, BSZ)
    # critics: 2 NC online forwards ((obs, act) and (obs, act_)), NC target forwards on (next_obs, next_act), NC backwards;
    # actor: forwards on obs and on next_obs, one backward
    total = 3 * NC * qf + NC * (qw + qx) + 2 * pf + pw + px
    return total / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import border_amd as B
    import awac_restatement as R
    spec = R.AwacSpec(O, A, UNITS, UNITS, n_critics=NC)
    rng = np.random.default_rng(0)
    n = 50_000
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=n, seed=42), (O,), np.float32, (A,), np.float32)
    rb.push(rng.standard_normal((n, O)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
            rng.standard_normal((n, O)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))
    agent = B.Awac.build(spec.to_config(B, BSZ, device=0, seed=1, train=True))

    for _ in range(args.warmup):
        agent.opt(rb)
    agent.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        agent.opt(rb)
    agent.sync()
    timed = time.perf_counter() - t0

    legs = []
    for _ in range(args.legs):
        k, t0 = 0, time.perf_counter()
        while True:
            for _ in range(50):
                agent.opt(rb)
            k += 50
            agent.sync()
            el = time.perf_counter() - t0
            if el >= 0.3:
                break
        legs.append(k / el)
    rec = agent.opt_with_record(rb)

    # launches per update: one profile bracket per launch of the update ("sample" = the replay buffer's gather)
    from bench import read_profile
    agent.profile_enable(True)
    agent.opt(rb)
    agent.sync()
    slots = read_profile(agent)
    agent.profile_enable(False)
    launches = sum(1 for l, _ in slots if l not in ("sample", "_null"))
    kernel_ms = sum(v for l, v in slots if l not in ("sample", "_null"))
    agent.close(); rb.close()

    cpu_rate = None
    if not args.no_cpu:
        import torch
        torch.set_num_threads(16)
        ref = R.AwacRestatement(spec, *spec.init_params(1))
        batch = R.make_batch(spec, BSZ, 3)
        z = spec.draws(BSZ, 4)
        ref.update(*batch, *z)
        t0 = time.perf_counter()
        for _ in range(args.cpu_steps):
            ref.update(*batch, *z)
        cpu_rate = args.cpu_steps / (time.perf_counter() - t0)

    gf = update_gflop()
    ups = args.steps / timed
    legs_sorted = sorted(legs)
    out = {
        "metric": "awac_pen_updates_per_s", "shape": {"obs": O, "act": A, "units": list(UNITS), "n_critics": NC, "batch": BSZ},
        "warmup": args.warmup, "steps": args.steps, "value": round(ups, 1), "ms_per_update": round(1e3 / ups, 4),
        "steady_legs_updates_per_s": [round(x, 1) for x in legs], "steady_median": round(legs_sorted[len(legs) // 2], 1),
        "steady_spread_pct": round(100.0 * (legs_sorted[-1] - legs_sorted[0]) / legs_sorted[len(legs) // 2], 2),
        "launches_per_update": launches, "profiled_kernel_ms_per_update": round(kernel_ms, 4),
        "gflop_per_update": round(gf, 4), "fp32_peak_share_pct": round(100.0 * gf * ups / (PEAK_FP32_MFMA_TFLOPS * 1e3), 3),
        "restatement_cpu16_updates_per_s": None if cpu_rate is None else round(cpu_rate, 2),
        "record": {k: round(float(v), 6) for k, v in rec.items()},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
