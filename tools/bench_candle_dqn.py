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

--cnn --act: per-call latency of `sample` on host frame stacks (the call of the online loop: rows to the device, the forward, the
action back) at n = 1 and n = 8 on the act paths "layers" and "image" (csrc/cnn_act_img.hpp), ONE agent, the paths alternating in
one process: after a warm-up of both, five rounds of 1 000 calls per path; median and spread of the rounds, and the per-launch times
of one call from the profile brackets.  Writes profiles/bench_candle_dqn_cnn_act.json.  The bar: at n = 1 the worst "image" round is
not slower than the best "layers" round of the same run.

--cnn --arithmetic both: the candle agent as built ("f32_exact") and after set_arithmetic("bf16x3_6"), legs alternating in one process, no tch agent,
at B = 32 and B = 256; writes profiles/bench_candle_dqn_cnn_b3.json and says whether the worst split leg beats the best exact leg.
With --act: exact layers, exact image, split layers, split image alternating at n = 1 and 8 (profiles/bench_candle_dqn_cnn_act_b3.json).
--arithmetic f32_exact | bf16x3_6 alone sets that arithmetic on the candle agent of the other runs.  No speed bar.

--cnn --head-form both: the candle agent as built ("layers") and after set_head_form("splitk") (csrc/cdqn_head_fwd.hpp), legs alternating
in one process, no tch agent, at B = 32 and B = 256; writes profiles/bench_candle_dqn_cnn_headform.json.  The bar, at B = 32 only: the
worst "splitk" leg is not below the best "layers" leg.  With --act: `sample` on the layer act path under both head forms alternating
at n = 1 and 8 (profiles/bench_candle_dqn_cnn_act_headform.json).  --head-form splitk alone sets the form on the candle agent of
--cnn and --cnn --act.

--cnn --head-bwd both: the candle agent as built ("layers") and after set_head_bwd_form("fused") (csrc/cdqn_head_bwd.hpp), legs
alternating in one process, no tch agent, at B = 32 and B = 256; writes --out, by default profiles/bench_candle_dqn_cnn_headbwd.json
(..._headbwd_splitk.json with --head-form splitk).  No speed bar.  --head-bwd fused alone sets the form on the candle agent of --cnn;
--head-form and --arithmetic (not "both") apply to both agents.  --against-parent PARENT_DIR TREE_DIR merges the b32.json / b256.json
that `--cnn --no-tch --batch 32 | 256 > <dir>/b<batch>.json` of a parent checkout and of this tree left into
profiles/bench_candle_dqn_cnn_headbwd_parent.json (needs no device).
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
    ap.add_argument("--act", action="store_true", help="--cnn: the acting-call latency of the act paths instead of the update rate")
    ap.add_argument("--arithmetic", choices=("f32_exact", "bf16x3_6", "both"), default="f32_exact", help="--cnn: the candle agent's arithmetic; both: exact against split")
    ap.add_argument("--head-form", choices=("layers", "splitk", "both"), default="layers", help="--cnn: the candle agent's head forward; both: layers against splitk")
    ap.add_argument("--head-bwd", choices=("layers", "fused", "both"), default="layers", help="--cnn: the candle agent's head backward; both: layers against fused")
    ap.add_argument("--against-parent", nargs=2, metavar=("PARENT_DIR", "TREE_DIR"), default=None,
                    help="merge <dir>/b32.json and <dir>/b256.json (the output of --cnn --no-tch --batch 32 | 256 of a parent checkout and of this tree) into one record")
    args = ap.parse_args()
    if args.against_parent:
        return merge_against_parent(args)
    if args.cnn and args.head_bwd == "both":
        if args.out is None:
            args.out = os.path.join(ROOT, "profiles", "bench_candle_dqn_cnn_headbwd" + ("_splitk" if args.head_form == "splitk" else "") + ".json")
        return main_cnn_headbwd(args)
    if args.out is None:
        stem = "bench_candle_dqn" if not args.cnn else "bench_candle_dqn_cnn" + ("" if args.batch == 32 else f"_b{args.batch}")
        args.out = os.path.join(ROOT, "profiles", stem + ".json")
    if args.cnn and args.head_form == "both":
        return main_cnn_act_headform(args) if args.act else main_cnn_headform(args)
    if args.cnn and args.act:
        return main_cnn_act(args)
    if args.cnn and args.arithmetic == "both":
        return main_cnn_both(args)
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
    if args.arithmetic != "f32_exact":   # (the exact line is an agent nobody touched)
        pairs[0][1].set_arithmetic(args.arithmetic)
    pairs[0][1].set_head_form(args.head_form)
    if args.head_bwd != "layers":        # (the layers line is an agent nobody touched)
        pairs[0][1].set_head_bwd_form(args.head_bwd)
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


def main_cnn_both(args):
    import border_amd as B
    import candle_dqn_cnn_restatement as RC
    NS, NA, ARITH = 4, 6, ("f32_exact", "bf16x3_6")
    spec = RC.CandleDqnCnnSpec(NS, NA, lr=1e-3, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01), double_dqn=args.double_dqn)
    out = {"metric": "dqn_atari_candle_updates_per_s_by_arithmetic", "shape": {"n_stack": NS, "n_actions": NA, "opt": "AdamW", "loss": "Mse",
                                                                                "double_dqn": bool(args.double_dqn)}, "warmup": args.warmup, "steps": args.steps}
    for bsz in (32, 256):
        pairs = [(ar, B.CandleDqn.build(spec.to_config(B, bsz, device=0, seed=1)), ring_u8(B, NS)) for ar in ARITH]
        pairs[1][1].set_arithmetic(ARITH[1])
        res = {ar: {"value": round(window(agent, rb, args.warmup, args.steps), 1)} for ar, agent, rb in pairs}
        legs = {ar: [] for ar in ARITH}
        for _ in range(args.legs):
            for ar, agent, rb in pairs:
                legs[ar].append(leg(agent, rb))
        for ar, agent, rb in pairs:
            v = sorted(legs[ar])
            res[ar].update(ms_per_update=round(1e3 / res[ar]["value"], 4), steady_legs_updates_per_s=[round(x, 1) for x in legs[ar]],
                           steady_median=round(v[len(v) // 2], 1), steady_spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2), **launches(agent, rb))
            agent.close(); rb.close()
        res["split_over_exact_steady_median"] = round(res["bf16x3_6"]["steady_median"] / res["f32_exact"]["steady_median"], 4)
        res["worst_split_leg_beats_best_exact_leg"] = bool(min(legs["bf16x3_6"]) > max(legs["f32_exact"]))
        out[f"b{bsz}"] = res
    out["value"] = out["b32"]["bf16x3_6"]["value"]
    line = json.dumps(out)
    path = os.path.join(ROOT, "profiles", "bench_candle_dqn_cnn_b3.json")
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


def main_cnn_headform(args):
    """layers against splitk: one agent per head form (both of --arithmetic, "both" excepted), legs alternating, B = 32 and 256"""
    import border_amd as B
    import candle_dqn_cnn_restatement as RC
    NS, NA, FORMS = 4, 6, ("layers", "splitk")
    spec = RC.CandleDqnCnnSpec(NS, NA, lr=1e-3, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01), double_dqn=args.double_dqn)
    arith = "f32_exact" if args.arithmetic == "both" else args.arithmetic
    out = {"metric": "dqn_atari_candle_updates_per_s_by_head_form", "shape": {"n_stack": NS, "n_actions": NA, "opt": "AdamW", "loss": "Mse", "arithmetic": arith,
                                                                               "double_dqn": bool(args.double_dqn)}, "warmup": args.warmup, "steps": args.steps}
    for bsz in (32, 256):
        pairs = [(hf, B.CandleDqn.build(spec.to_config(B, bsz, device=0, seed=1)), ring_u8(B, NS)) for hf in FORMS]
        for hf, agent, _ in pairs:
            if arith != "f32_exact":
                agent.set_arithmetic(arith)
            agent.set_head_form(hf)
        res = {hf: {"value": round(window(agent, rb, args.warmup, args.steps), 1)} for hf, agent, rb in pairs}
        legs = {hf: [] for hf in FORMS}
        for _ in range(args.legs):
            for hf, agent, rb in pairs:
                legs[hf].append(leg(agent, rb))
        for hf, agent, rb in pairs:
            v = sorted(legs[hf])
            res[hf].update(ms_per_update=round(1e3 / res[hf]["value"], 4), steady_legs_updates_per_s=[round(x, 1) for x in legs[hf]],
                           steady_median=round(v[len(v) // 2], 1), steady_spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2), **launches(agent, rb))
            agent.close(); rb.close()
        res["splitk_over_layers_steady_median"] = round(res["splitk"]["steady_median"] / res["layers"]["steady_median"], 4)
        res["worst_splitk_leg_not_below_best_layers_leg"] = bool(min(legs["splitk"]) >= max(legs["layers"]))
        out[f"b{bsz}"] = res
    out["value"] = out["b32"]["splitk"]["value"]
    line = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "bench_candle_dqn_cnn_headform.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def main_cnn_headbwd(args):
    """head backward layers against fused: one agent per form (both of --arithmetic and --head-form, "both" excepted), legs alternating, B = 32 and 256"""
    import border_amd as B
    import candle_dqn_cnn_restatement as RC
    NS, NA, FORMS = 4, 6, ("layers", "fused")
    spec = RC.CandleDqnCnnSpec(NS, NA, lr=1e-3, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01), double_dqn=args.double_dqn)
    arith = "f32_exact" if args.arithmetic == "both" else args.arithmetic
    head = "layers" if args.head_form == "both" else args.head_form
    out = {"metric": "dqn_atari_candle_updates_per_s_by_head_bwd_form", "shape": {"n_stack": NS, "n_actions": NA, "opt": "AdamW", "loss": "Mse", "arithmetic": arith,
                                                                                   "head_form": head, "double_dqn": bool(args.double_dqn)},
           "warmup": args.warmup, "steps": args.steps}
    for bsz in (32, 256):
        pairs = [(hb, B.CandleDqn.build(spec.to_config(B, bsz, device=0, seed=1)), ring_u8(B, NS)) for hb in FORMS]
        for hb, agent, _ in pairs:
            if arith != "f32_exact":
                agent.set_arithmetic(arith)
            agent.set_head_form(head)
            agent.set_head_bwd_form(hb)
        res = {hb: {"value": round(window(agent, rb, args.warmup, args.steps), 1)} for hb, agent, rb in pairs}
        legs = {hb: [] for hb in FORMS}
        for _ in range(args.legs):
            for hb, agent, rb in pairs:
                legs[hb].append(leg(agent, rb))
        for hb, agent, rb in pairs:
            v = sorted(legs[hb])
            res[hb].update(ms_per_update=round(1e3 / res[hb]["value"], 4), steady_legs_updates_per_s=[round(x, 1) for x in legs[hb]],
                           steady_median=round(v[len(v) // 2], 1), steady_spread_pct=round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2), **launches(agent, rb))
            agent.close(); rb.close()
        res["fused_over_layers_steady_median"] = round(res["fused"]["steady_median"] / res["layers"]["steady_median"], 4)
        res["worst_fused_leg_not_below_best_layers_leg"] = bool(min(legs["fused"]) >= max(legs["layers"]))
        out[f"b{bsz}"] = res
    out["value"] = out["b32"]["fused"]["value"]
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


def merge_against_parent(args):
    """the layers agent of a parent checkout against this tree's: the output of four runs `--cnn --no-tch --batch b > <dir>/b<b>.json`,
    taken alternating in one sitting, as one record (--out, or profiles/bench_candle_dqn_cnn_headbwd_parent.json)"""
    out = {"metric": "dqn_atari_candle_updates_per_s_layers_agent_parent_against_tree",
           "note": "tools/bench_candle_dqn.py --cnn --no-tch of the parent commit and of this tree, alternating in one sitting on one MI355X"}
    for b in (32, 256):
        for who, d in zip(("parent", "tree"), args.against_parent):
            with open(os.path.join(d, f"b{b}.json")) as f:
                out[f"{who}_b{b}"] = json.loads(next(l for l in f if l.startswith("{")))["candle_dqn_cnn"]
        out[f"tree_over_parent_steady_median_b{b}"] = round(out[f"tree_b{b}"]["steady_median"] / out[f"parent_b{b}"]["steady_median"], 4)
    line = json.dumps(out)
    with open(args.out or os.path.join(ROOT, "profiles", "bench_candle_dqn_cnn_headbwd_parent.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def main_cnn_act_headform(args, rounds=5, calls=1000):
    """`sample` on the layer act path, head form layers against splitk: one agent per form, alternating round by round, n = 1 and 8"""
    import border_amd as B
    import candle_dqn_cnn_restatement as RC
    from bench import read_profile
    NS, NA, FORMS = 4, 6, ("layers", "splitk")
    spec = RC.CandleDqnCnnSpec(NS, NA, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01))
    arith = "f32_exact" if args.arithmetic == "both" else args.arithmetic
    def build(hf):
        a = B.CandleDqn.build(spec.to_config(B, 32, device=0, seed=1, train=True, explorer=B.EpsilonGreedy(eps_start=0.02, eps_final=0.02, final_step=1)))
        if arith != "f32_exact":
            a.set_arithmetic(arith)
        a.set_act_path("layers")
        a.set_head_form(hf)
        return a
    agents = {hf: build(hf) for hf in FORMS}
    res = {}
    for n in (1, 8):
        obs = np.random.default_rng(n).integers(0, 256, (n, 84 * 84 * NS), dtype=np.uint8)
        us = {hf: [] for hf in FORMS}
        for hf in FORMS:
            for _ in range(200):
                agents[hf].sample(obs)
        for _ in range(rounds):
            for hf in FORMS:
                t0 = time.perf_counter()
                for _ in range(calls):
                    agents[hf].sample(obs)
                us[hf].append(1e6 * (time.perf_counter() - t0) / calls)
        r = {}
        for hf in FORMS:
            v = sorted(us[hf])
            b = build(hf)   # (an agent of its own: profile slots keep the names of their first use)
            for _ in range(20):
                b.sample(obs)
            b.profile_enable(True)
            for _ in range(100):
                b.sample(obs)
            slots = read_profile(b)
            b.profile_enable(False)
            b.close()
            r[hf] = {"us_per_call_rounds": [round(x, 2) for x in us[hf]], "median_us": round(v[len(v) // 2], 2),
                     "spread_pct": round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2), "best_us": round(v[0], 2), "worst_us": round(v[-1], 2),
                     "profile_brackets_us": [[l, round(1e3 * ms, 2)] for l, ms in slots if l != "_null"]}
        r["splitk_over_layers_median"] = round(r["splitk"]["median_us"] / r["layers"]["median_us"], 4)
        r["worst_splitk_not_slower_than_best_layers"] = bool(r["splitk"]["worst_us"] <= r["layers"]["best_us"])
        res[f"n{n}"] = r
    for a in agents.values():
        a.close()
    out = {"metric": "dqn_atari_candle_sample_us_per_call_by_head_form", "shape": {"n_stack": NS, "n_actions": NA, "rows": "host u8", "act_path": "layers",
                                                                                    "arithmetic": arith}, "rounds": rounds,
           "calls_per_round": calls, "value": res["n1"]["splitk"]["median_us"], **res}
    line = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "bench_candle_dqn_cnn_act_headform.json"), "w") as f:
        f.write(line + "\n")
    print(line)


def main_cnn_act(args, rounds=5, calls=1000):
    import border_amd as B
    import candle_dqn_cnn_restatement as RC
    from bench import read_profile
    NS, NA, PATHS = 4, 6, ("layers", "image")
    spec = RC.CandleDqnCnnSpec(NS, NA, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01))
    if args.arithmetic == "both":
        return main_cnn_act_both(args, spec, rounds, calls)
    def build():
        a = B.CandleDqn.build(spec.to_config(B, 32, device=0, seed=1, train=True, explorer=B.EpsilonGreedy(eps_start=0.02, eps_final=0.02, final_step=1)))
        if args.arithmetic != "f32_exact":
            a.set_arithmetic(args.arithmetic)
        a.set_head_form(args.head_form)
        return a
    a = build()
    res = {}
    for n in (1, 8):
        obs = np.random.default_rng(n).integers(0, 256, (n, 84 * 84 * NS), dtype=np.uint8)
        us = {p: [] for p in PATHS}
        for p in PATHS:   # warm-up of both paths: code objects, the path's buffers
            a.set_act_path(p)
            for _ in range(200):
                a.sample(obs)
        for _ in range(rounds):
            for p in PATHS:
                a.set_act_path(p)
                t0 = time.perf_counter()
                for _ in range(calls):
                    a.sample(obs)   # (returns with the actions on the host: the call is synchronous)
                us[p].append(1e6 * (time.perf_counter() - t0) / calls)
        r = {}
        for p in PATHS:
            v = sorted(us[p])
            b = build()   # (an agent of its own per path: profile slots keep the names of their first use)
            b.set_act_path(p)
            for _ in range(20):
                b.sample(obs)
            b.profile_enable(True)
            for _ in range(100):
                b.sample(obs)
            slots = read_profile(b)
            b.profile_enable(False)
            b.close()
            r[p] = {"us_per_call_rounds": [round(x, 2) for x in us[p]], "median_us": round(v[len(v) // 2], 2),
                    "spread_pct": round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2), "best_us": round(v[0], 2), "worst_us": round(v[-1], 2),
                    "profile_brackets_us": [[l, round(1e3 * ms, 2)] for l, ms in slots if l != "_null"]}
        r["image_over_layers_median"] = round(r["image"]["median_us"] / r["layers"]["median_us"], 4)
        r["worst_image_not_slower_than_best_layers"] = bool(r["image"]["worst_us"] <= r["layers"]["best_us"])
        res[f"n{n}"] = r
    a.close()
    out = {"metric": "dqn_atari_candle_sample_us_per_call", "shape": {"n_stack": NS, "n_actions": NA, "rows": "host u8"}, "rounds": rounds,
           "calls_per_round": calls, "value": res["n1"]["image"]["median_us"], **res}
    line = json.dumps(out)
    path = os.path.join(ROOT, "profiles", "bench_candle_dqn_cnn_act.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


def main_cnn_act_both(args, spec, rounds, calls):
    """exact layers, exact image, split layers, split image: one agent per arithmetic, the four forms alternating round by round"""
    import border_amd as B
    from bench import read_profile
    NS, NA = spec.n_stack, spec.n_actions
    FORMS = [(ar, p) for ar in ("f32_exact", "bf16x3_6") for p in ("layers", "image")]
    def build(ar):
        a = B.CandleDqn.build(spec.to_config(B, 32, device=0, seed=1, train=True, explorer=B.EpsilonGreedy(eps_start=0.02, eps_final=0.02, final_step=1)))
        if ar != "f32_exact":
            a.set_arithmetic(ar)
        return a
    agents = {ar: build(ar) for ar in ("f32_exact", "bf16x3_6")}
    res = {}
    for n in (1, 8):
        obs = np.random.default_rng(n).integers(0, 256, (n, 84 * 84 * NS), dtype=np.uint8)
        us = {f: [] for f in FORMS}
        for ar, p in FORMS:
            agents[ar].set_act_path(p)
            for _ in range(200):
                agents[ar].sample(obs)
        for _ in range(rounds):
            for ar, p in FORMS:
                agents[ar].set_act_path(p)
                t0 = time.perf_counter()
                for _ in range(calls):
                    agents[ar].sample(obs)
                us[(ar, p)].append(1e6 * (time.perf_counter() - t0) / calls)
        r = {}
        for ar, p in FORMS:
            v = sorted(us[(ar, p)])
            b = build(ar)
            b.set_act_path(p)
            for _ in range(20):
                b.sample(obs)
            b.profile_enable(True)
            for _ in range(100):
                b.sample(obs)
            slots = read_profile(b)
            b.profile_enable(False)
            b.close()
            r[f"{ar}_{p}"] = {"us_per_call_rounds": [round(x, 2) for x in us[(ar, p)]], "median_us": round(v[len(v) // 2], 2),
                              "spread_pct": round(100.0 * (v[-1] - v[0]) / v[len(v) // 2], 2), "best_us": round(v[0], 2), "worst_us": round(v[-1], 2),
                              "profile_brackets_us": [[l, round(1e3 * ms, 2)] for l, ms in slots if l != "_null"]}
        for p in ("layers", "image"):
            r[f"worst_split_{p}_beats_best_exact_{p}"] = bool(r[f"bf16x3_6_{p}"]["worst_us"] < r[f"f32_exact_{p}"]["best_us"])
        r["worst_split_image_beats_best_split_layers"] = bool(r["bf16x3_6_image"]["worst_us"] < r["bf16x3_6_layers"]["best_us"])
        res[f"n{n}"] = r
    for a in agents.values():
        a.close()
    out = {"metric": "dqn_atari_candle_sample_us_per_call_by_arithmetic", "shape": {"n_stack": NS, "n_actions": NA, "rows": "host u8"}, "rounds": rounds,
           "calls_per_round": calls, "value": res["n1"]["bf16x3_6_image"]["median_us"], **res}
    line = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "bench_candle_dqn_cnn_act_b3.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
