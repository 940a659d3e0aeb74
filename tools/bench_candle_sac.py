"""candle SAC update rate (csrc/candle_sac.hip): Agent::opt over an HBM replay ring in train mode (a and next_a drawn from the
device stream, as under Trainer, which calls agent.train()).  Prints ONE JSON line per workload:

  pendulum   examples/gym/sac_pendulum: obs 3, act 1, [64, 64] for the Mlp2 actor and the twin critics, Tanh{2}, Auto, B = 128
  pen        obs 45, act 24, [256, 256] Mlp2 actor, [256, 256] twin critics, Tanh, Auto, B = 256
  awac       tools/bench_awac.py's workload in the same job on the same box: the yardstick (its own JSON line, unchanged)

  W untimed updates; K timed updates (device-synchronised wall clock); a steady leg of >= 0.3 s repeated `--legs` times (the spread);
  launches per update and their names from the agent's profile brackets (bdr_agent_profile_*), with the largest bracket that is not
  a dense layer; the float32 autograd restatement's rate on 16 CPU threads, for context.

  python tools/bench_candle_sac.py --steps 300 --warmup 20
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = {
    "pendulum": dict(O=3, A=1, p_units=(64, 64), q_units=(64, 64), bsz=128, scale=2.0, target_entropy=-1.0),
    "pen": dict(O=45, A=24, p_units=(256, 256), q_units=(256, 256), bsz=256, scale=1.0, target_entropy=-24.0),
}
DENSE = ("pi_fwd", "q_fwd", "q_tgt_fwd", "q_dx", "pi_bwd_adam", "q_bwd_adam_track")   # brackets of dense.hpp's kernels


def run(name, w, args):
    import border_amd as B
    import candle_sac_restatement as R
    O, A, bsz = w["O"], w["A"], w["bsz"]
    spec = R.CandleSacSpec(O, A, w["p_units"], w["q_units"], actor_kind="Mlp2", action_limit="Tanh", action_scale=w["scale"],
                           ent_coef=("Auto", w["target_entropy"], 3e-4))
    rng = np.random.default_rng(0)
    n = 50_000
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=n, seed=42), (O,), np.float32, (A,), np.float32)
    rb.push(rng.standard_normal((n, O)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
            rng.standard_normal((n, O)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))
    agent = B.CandleSac.build(spec.to_config(B, bsz, device=0, seed=1, train=True))

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

    from bench import read_profile
    agent.profile_enable(True)
    agent.opt(rb)
    agent.sync()
    slots = [(l, v) for l, v in read_profile(agent) if l not in ("sample", "_null")]
    agent.profile_enable(False)
    agent.close(); rb.close()
    per_name = {}
    for l, v in slots:
        per_name[l] = per_name.get(l, 0.0) + v
    own = {l: v for l, v in per_name.items() if l not in DENSE}
    largest = max(own, key=own.get) if own else None

    cpu_rate = None
    if not args.no_cpu:
        import torch
        torch.set_num_threads(16)
        ref = R.CandleSacRestatement(spec, *spec.init_params(1))
        batch = R.make_batch(spec, bsz, 3)
        z = spec.draws(bsz, 4, 0.3)
        ref.update(*batch, *z)
        t0 = time.perf_counter()
        for _ in range(args.cpu_steps):
            ref.update(*batch, *z)
        cpu_rate = args.cpu_steps / (time.perf_counter() - t0)

    ups = args.steps / timed
    ls = sorted(legs)
    return {
        "metric": f"candle_sac_{name}_updates_per_s",
        "shape": {"obs": O, "act": A, "p_units": list(w["p_units"]), "q_units": list(w["q_units"]), "n_critics": 2, "batch": bsz, "actor": "Mlp2"},
        "warmup": args.warmup, "steps": args.steps, "value": round(ups, 1), "ms_per_update": round(1e3 / ups, 4),
        "steady_legs_updates_per_s": [round(x, 1) for x in legs], "steady_median": round(ls[len(ls) // 2], 1),
        "steady_spread_pct": round(100.0 * (ls[-1] - ls[0]) / ls[len(ls) // 2], 2),
        "launches_per_update": len(slots), "launch_names": [l for l, _ in slots],
        "profiled_kernel_ms_per_update": round(sum(v for _, v in slots), 4),
        "profiled_ms_by_bracket": {l: round(v, 4) for l, v in per_name.items()}, "largest_non_dense_bracket": largest,
        "restatement_cpu16_updates_per_s": None if cpu_rate is None else round(cpu_rate, 2),
        "record": {k: round(float(v), 6) for k, v in rec.items()},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-awac", action="store_true")
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    args = ap.parse_args()
    for name, w in WORKLOADS.items():
        if args.only in (None, name):
            print(json.dumps(run(name, w, args)), flush=True)
    if not args.no_awac and args.only is None:   # the yardstick, a fresh process on the same box
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_awac.py"), "--steps", str(args.steps), "--warmup", str(args.warmup), "--legs", str(args.legs)]
        print(subprocess.run(cmd + (["--no-cpu"] if args.no_cpu else []), check=True, capture_output=True, text=True).stdout.strip(), flush=True)


if __name__ == "__main__":
    main()
