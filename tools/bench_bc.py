"""BC update rate at the shape of examples/d4rl/bc_pen (obs 45, act 24, policy Mlp [256, 256] with a Tanh output, B = 256): Agent::opt
over an HBM replay ring holding an offline dataset.  Prints ONE JSON line.

  W untimed updates; K timed updates (device-synchronised wall clock); a steady leg of >= 0.3 s repeated `--legs` times (the spread);
  launches per update from the agent's profile brackets (bdr_agent_profile_*); algorithmic GFLOP per update and the share of the FP32
  MFMA peak; the float32 autograd restatement's rate on 16 CPU threads, for context.

  python tools/bench_bc.py --steps 300 --warmup 30 --kernel-form general|fused|fused_mfma [--head-rows 8|16|32]
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
O, A, UNITS, BSZ = 45, 24, (256, 256), 256


def update_gflop():
    """forward + weight gradient + input gradient (without layer 0) multiply-add FLOPs of one update"""
    dims = [O] + list(UNITS) + [A]
    mac = [dims[k] * dims[k + 1] for k in range(len(dims) - 1)]
    f = 2 * BSZ * sum(mac)
    return (3 * f - 2 * BSZ * mac[0]) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--kernel-form", choices=("default", "general", "fused", "fused_mfma"), default="default")
    ap.add_argument("--head-rows", type=int, default=0)
    args = ap.parse_args()

    import border_amd as B
    import bc_restatement as R
    spec = R.BcSpec(O, A, UNITS, "Tanh", lr=1e-3, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01))
    rng = np.random.default_rng(0)
    n = 50_000
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=n, seed=42), (O,), np.float32, (A,), np.float32)
    rb.push(rng.standard_normal((n, O)).astype(np.float32), rng.uniform(-0.95, 0.95, (n, A)).astype(np.float32),
            rng.standard_normal((n, O)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))
    agent = B.Bc.build(spec.to_config(B, BSZ, device=0, seed=1, kernel_form=args.kernel_form, head_rows=args.head_rows))

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
    per_bracket = [[l, round(v, 4)] for l, v in slots if l != "_null"]
    agent.close(); rb.close()

    cpu_rate = None
    if not args.no_cpu:
        import torch
        torch.set_num_threads(16)
        ref = R.BcRestatement(spec, spec.init_params(1))
        batch = R.make_batch(spec, BSZ, 3)
        ref.update(*batch)
        t0 = time.perf_counter()
        for _ in range(args.cpu_steps):
            ref.update(*batch)
        cpu_rate = args.cpu_steps / (time.perf_counter() - t0)

    gf = update_gflop()
    ups = args.steps / timed
    legs_sorted = sorted(legs)
    out = {
        "metric": "bc_pen_updates_per_s", "shape": {"obs": O, "act": A, "units": list(UNITS), "activation_out": "Tanh", "batch": BSZ},
        "kernel_form": args.kernel_form, "head_rows": args.head_rows,
        "warmup": args.warmup, "steps": args.steps, "value": round(ups, 1), "ms_per_update": round(1e3 / ups, 4),
        "steady_legs_updates_per_s": [round(x, 1) for x in legs], "steady_median": round(legs_sorted[len(legs) // 2], 1),
        "steady_spread_pct": round(100.0 * (legs_sorted[-1] - legs_sorted[0]) / legs_sorted[len(legs) // 2], 2),
        "launches_per_update": launches, "launches_per_update_with_gather": launches + sum(1 for l, _ in slots if l == "sample"),
        "profiled_kernel_ms_per_update": round(kernel_ms, 4), "profile_brackets_ms": per_bracket,
        "gflop_per_update": round(gf, 4), "fp32_peak_share_pct": round(100.0 * gf * ups / (PEAK_FP32_MFMA_TFLOPS * 1e3), 3),
        "restatement_cpu16_updates_per_s": None if cpu_rate is None else round(cpu_rate, 2),
        "record": {k: round(float(v), 6) for k, v in rec.items()},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
