"""Acting latency of the dense-agent agents at the pen shape (examples/d4rl/{iql,bc}_pen: obs 45 float64, act 24): one
Policy::sample on raw environment rows with the dataset's normaliser (bdr_agent_sample_raw), the call the Evaluator makes once per
environment step.  Prints one JSON line per (agent, rows) and writes them to --out.

  IQL: actor Mlp3 [256, 256, 256] (four layers); BC: policy Mlp [256, 256] with a Tanh output (three layers).
  n = 1 (the evaluator's call), 32 and 256 rows; float64 host rows; the layer path (the parent commit's code) against k_dense_act.
  Both paths run in ONE process on two agents built from the same parameters, in `--rounds` alternating rounds: layers, fused,
  layers, fused, ...; a round times `--calls` synchronous calls (each returns the action to the host, so the host clock around a
  call is the call's latency) after `--warmup` untimed ones.  Per path: the median call of every round, and the spread of those
  medians between rounds.  "fused_faster_in_every_round": every fused round median is below every layer round median by more than
  the larger spread - the rule by which a default is changed.  The actions of the two paths are compared bit
  for bit on the timed rows before anything is timed.

  python tools/bench_act.py --calls 2000 --warmup 200 --rounds 5 [--out profiles/bench_act_pen.json]
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

O, A = 45, 24


def build(B, kind, path):
    if kind == "iql":
        import iql_restatement as R
        spec = R.IqlSpec(O, A, (256, 256), (256, 256, 256), (256, 256))
        p = spec.init_params(1)
        a = B.Iql.build(spec.to_config(B, 256, device=0, seed=1))
        a.set_params(p[0], "actor")
        units = [256, 256, 256]
    else:
        import bc_restatement as R
        spec = R.BcSpec(O, A, (256, 256), "Tanh")
        a = B.Bc.build(spec.to_config(B, 256, device=0, seed=1))
        a.set_params(spec.init_params(1))
        units = [256, 256]
    a.eval()
    a.set_act_path(path)
    return a, units


def round_us(agent, rows, norm, calls):
    t = np.empty(calls)
    for k in range(calls):
        t0 = time.perf_counter()
        agent.sample_raw(rows, norm)
        t[k] = time.perf_counter() - t0
    return 1e6 * float(np.median(t)), 1e6 * float(t.mean())


def launches(agent, rows, norm):
    agent.profile_enable(True)
    agent.sample_raw(rows, norm)
    names = [k for k, _ in agent.profile_read()]
    agent.profile_enable(False)
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 32, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import border_amd as B
    if B.device_count() == 0:
        raise SystemExit("no MI355X visible: acting latency is measured on the GPU")
    k = np.arange(O)
    mean, std = (0.05 * k).astype(np.float32), (0.5 + 0.25 * (k % 5)).astype(np.float32)
    norm = B.ObsNormalizer(O, 0).set(mean, std)
    lines = []
    for kind in ("iql", "bc"):
        agents = {path: build(B, kind, path) for path in ("layers", "fused")}
        units = agents["layers"][1]
        for n in args.rows:
            rows = mean.astype(np.float64) + std.astype(np.float64) * np.random.default_rng(n).standard_normal((n, O))
            same = bool((agents["layers"][0].sample_raw(rows, norm).view(np.uint32) == agents["fused"][0].sample_raw(rows, norm).view(np.uint32)).all())
            calls = max(50, args.calls // max(1, n // 32))
            for path in ("layers", "fused"):
                for _ in range(args.warmup):
                    agents[path][0].sample_raw(rows, norm)
            med = {"layers": [], "fused": []}
            avg = {"layers": [], "fused": []}
            for _ in range(args.rounds):
                for path in ("layers", "fused"):
                    m, a = round_us(agents[path][0], rows, norm, calls)
                    med[path].append(round(m, 2)); avg[path].append(round(a, 2))
            spread = {p: round(max(v) - min(v), 2) for p, v in med.items()}
            faster = min(med["layers"]) - max(med["fused"]) > max(spread.values())
            out = {
                "metric": "act_pen_sample_raw_us", "agent": kind, "shape": {"obs": O, "act": A, "units": units, "obs_dtype": "float64", "normaliser": True},
                "rows": n, "calls_per_round": calls, "warmup": args.warmup, "rounds": args.rounds, "bits_equal": same,
                "layers_round_median_us": med["layers"], "fused_round_median_us": med["fused"],
                "layers_round_mean_us": avg["layers"], "fused_round_mean_us": avg["fused"],
                "round_spread_us": spread, "fused_faster_in_every_round": bool(faster),
                "speedup_of_medians": round(float(np.median(med["layers"]) / np.median(med["fused"])), 3),
                "launches": {p: launches(agents[p][0], rows, norm) for p in ("layers", "fused")},
            }
            lines.append(out)
            print(json.dumps(out), flush=True)
        for a, _ in agents.values():
            a.close()
    norm.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
