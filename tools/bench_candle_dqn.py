"""Candle DQN update rate at the shape of examples/gym/dqn_cartpole (obs 4, 2 actions, Q-network Mlp [256, 256], B = 64, AdamW, Mse):
Agent::opt over an HBM replay ring, and the tch Dqn Mlp agent (border_amd.Dqn) at the same shape in the same process on the same
device, for comparison.  Prints ONE JSON line and writes it to profiles/bench_candle_dqn.json.

  per agent: W untimed updates; K timed updates (device-synchronised wall clock); a steady leg of >= 0.3 s repeated `--legs` times
  (the spread); launches per update from the agent's profile brackets (bdr_agent_profile_*).  The two agents' legs alternate.
  No speed threshold is set here: the figures go to README.md and DESIGN.md 17.

  python tools/bench_candle_dqn.py --steps 300 --warmup 30 [--double-dqn]

--cnn: the AtariCnn form at the shape of examples/atari/dqn_atari (n_stack 4, 6 actions, B = 32; --batch 256 is the C2 batch) over a
u8 ring, against the tch Dqn CNN agent built with arithmetic = "f32_exact" (the same products), legs alternating in the same
process; writes profiles/bench_candle_dqn_cnn.json (B = 32) or profiles/bench_candle_dqn_cnn_b256.json.  --no-tch runs the candle
agent alone (the kernel-trace run).
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

O, A, UNITS, BSZ = 4, 2, (256, 256), 64


def ring(B, n=50_000):
    rng = np.random.default_rng(0)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=n, seed=42), (O,), np.float32, (1,), np.int64)
    rb.push(rng.standard_normal((n, O)).astype(np.float32), rng.integers(0, A, (n, 1)).astype(np.int64),
            rng.standard_normal((n, O)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))
    return rb


def ring_u8(B, n_stack, n=2048):
    rng = np.random.default_rng(0)
    w = 84 * 84 * n_stack
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=n, seed=42), (w,), np.uint8, (1,), np.int64)
    rb.push(rng.integers(0, 256, (n, w), dtype=np.uint8), rng.integers(0, 6, (n, 1)).astype(np.int64),
            rng.integers(0, 256, (n, w), dtype=np.uint8), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))
    return rb


def leg(agent, rb):
    k, t0 = 0, time.perf_counter()
    while True:
        for _ in range(50):
            agent.opt(rb)
        k += 50
        agent.sync()
        el = time.perf_counter() - t0
        if el >= 0.3:
            return k / el


def window(agent, rb, warmup, steps):
    for _ in range(warmup):
        agent.opt(rb)
    agent.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        agent.opt(rb)
    agent.sync()
    return steps / (time.perf_counter() - t0)


def launches(agent, rb):
    from bench import read_profile
    agent.profile_enable(True)
    agent.opt(rb)
    agent.sync()
    slots = read_profile(agent)
    agent.profile_enable(False)
    n = sum(1 for l, _ in slots if l not in ("sample", "_null"))
    return {"launches_per_update": n, "launches_per_update_with_gather": n + sum(1 for l, _ in slots if l == "sample"),
            "profiled_kernel_ms_per_update": round(sum(v for l, v in slots if l not in ("sample", "_null")), 4),
            "profile_brackets_ms": [[l, round(v, 4)] for l, v in slots if l != "_null"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--double-dqn", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cnn", action="store_true")
    ap.add_argument("--batch", type=int, default=32, help="--cnn: 32 (dqn_atari) or 256 (the C2 batch)")
    ap.add_argument("--no-tch", action="store_true")
    args = ap.parse_args()
    if args.out is None:
        stem = "bench_candle_dqn" if not args.cnn else "bench_candle_dqn_cnn" + ("" if args.batch == 32 else f"_b{args.batch}")
        args.out = os.path.join(ROOT, "profiles", stem + ".json")
    if args.cnn:
        return main_cnn(args)

    import border_amd as B
    import candle_dqn_restatement as R
    spec = R.CandleDqnSpec(O, A, UNITS, lr=1e-3, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01), double_dqn=args.double_dqn)
    candle = B.CandleDqn.build(spec.to_config(B, BSZ, device=0, seed=1))
    tch = B.Dqn.build(B.DqnConfig(
        model_config=B.DqnModelConfig(B.MlpConfig(O, list(UNITS), A, False), B.OptimizerConfig.AdamW(1e-3, wd=0.01)),
        batch_size=BSZ, double_dqn=args.double_dqn, device=0, param_seed=1))
    rb_c, rb_t = ring(B), ring(B)

    res = {}
    for name, agent, rb in (("candle_dqn", candle, rb_c), ("tch_dqn_mlp", tch, rb_t)):
        res[name] = {"value": round(window(agent, rb, args.warmup, args.steps), 1), "legs": []}
    for _ in range(args.legs):   # alternating legs: both agents see the same machine state
        for name, agent, rb in (("candle_dqn", candle, rb_c), ("tch_dqn_mlp", tch, rb_t)):
            res[name]["legs"].append(leg(agent, rb))
    for name, agent, rb in (("candle_dqn", candle, rb_c), ("tch_dqn_mlp", tch, rb_t)):
        r, legs = res[name], sorted(res[name]["legs"])
        r["ms_per_update"] = round(1e3 / r["value"], 4)
        r["steady_legs_updates_per_s"] = [round(x, 1) for x in r.pop("legs")]
        r["steady_median"] = round(legs[len(legs) // 2], 1)
        r["steady_spread_pct"] = round(100.0 * (legs[-1] - legs[0]) / legs[len(legs) // 2], 2)
        r.update(launches(agent, rb))
    for x in (candle, tch, rb_c, rb_t):
        x.close()
    out = {"metric": "dqn_cartpole_updates_per_s", "shape": {"obs": O, "n_actions": A, "units": list(UNITS), "batch": BSZ, "opt": "AdamW", "loss": "Mse",
                                                              "double_dqn": bool(args.double_dqn)},
           "warmup": args.warmup, "steps": args.steps, "value": res["candle_dqn"]["value"],
           "candle_over_tch_steady_median": round(res["candle_dqn"]["steady_median"] / res["tch_dqn_mlp"]["steady_median"], 4), **res}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


def main_cnn(args):
    import border_amd as B
    import candle_dqn_cnn_restatement as RC
    NS, NA = 4, 6
    spec = RC.CandleDqnCnnSpec(NS, NA, lr=1e-3, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01), double_dqn=args.double_dqn)
    pairs = [("candle_dqn_cnn", B.CandleDqn.build(spec.to_config(B, args.batch, device=0, seed=1)), ring_u8(B, NS))]
    if not args.no_tch:
        tch = B.Dqn.build(B.DqnConfig(model_config=B.DqnModelConfig(B.AtariCnnConfig(NS, NA), B.OptimizerConfig.AdamW(1e-3, wd=0.01)),
                                      batch_size=args.batch, double_dqn=args.double_dqn, device=0, param_seed=1, arithmetic="f32_exact"))
        pairs.append(("tch_dqn_cnn_f32_exact", tch, ring_u8(B, NS)))
    res = {}
    for name, agent, rb in pairs:
        res[name] = {"value": round(window(agent, rb, args.warmup, args.steps), 1), "legs": []}
    for _ in range(args.legs):
        for name, agent, rb in pairs:
            res[name]["legs"].append(leg(agent, rb))
    for name, agent, rb in pairs:
        r, legs = res[name], sorted(res[name]["legs"])
        r["ms_per_update"] = round(1e3 / r["value"], 4)
        r["steady_legs_updates_per_s"] = [round(x, 1) for x in r.pop("legs")]
        if legs:
            r["steady_median"] = round(legs[len(legs) // 2], 1)
            r["steady_spread_pct"] = round(100.0 * (legs[-1] - legs[0]) / legs[len(legs) // 2], 2)
        if name == "candle_dqn_cnn":
            r.update(launches(agent, rb))
    for _, agent, rb in pairs:
        agent.close(); rb.close()
    out = {"metric": "dqn_atari_candle_updates_per_s", "shape": {"n_stack": NS, "n_actions": NA, "batch": args.batch, "opt": "AdamW", "loss": "Mse",
                                                                  "double_dqn": bool(args.double_dqn)},
           "warmup": args.warmup, "steps": args.steps, "value": res["candle_dqn_cnn"]["value"], **res}
    if not args.no_tch:
        out["candle_over_tch_steady_median"] = round(res["candle_dqn_cnn"]["steady_median"] / res["tch_dqn_cnn_f32_exact"]["steady_median"], 4)
    line = json.dumps(out)
    if not args.no_tch:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
