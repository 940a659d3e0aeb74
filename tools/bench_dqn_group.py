"""Aggregate member-updates/s of a DqnGroup (one launch per group step, one workgroup per member) against the same P standalone
agents stepped in a loop by Agent::opt, and group.sample against P sample calls - BASELINE config C1 (Mlp[64, 64], batch 32,
ring pre-filled) at P in {1, 8, 64, 256}, both sides in one process.

Protocol: warm-up, one window of K = 300 steps per side, then five legs of 0.3 s per side, the two sides alternating; the figure
is the median of the legs, the spread their min / max.  Writes one JSON document (default profiles/bench_dqn_group.json).

--online measures the online loop over a group instead (default profiles/bench_dqn_group_online.json), same protocol, host rows:
  push   group.push (one launch for P transitions) against a loop of P rb.push of one row, member-pushes/s
  iter   one online iteration group.sample -> group.push -> group.opt against the same iteration with the P rb.push calls in
         the middle (what an online loop over a group had to be before group.push), member-iterations/s
and states for every P whether the worst grouped leg beats the best leg of the loop form by more than the legs' min-max spread.

--per measures prioritized replay under a group (default profiles/bench_dqn_group_per.json): rings of 10 000 with PerConfig() defaults,
same protocol and bar:
  opt    group.opt of a group switched on (DqnGroup(prioritized=True)) against a loop of Agent::opt on the same kind of rings,
         member-updates/s
  iter   group.sample -> group.push -> group.opt against the same iteration with P rb.push calls in the middle, member-iterations/s

--eval measures the lockstep evaluator (default profiles/bench_dqn_group_eval.json): members in eval mode, a trivial environment with
episodes of a fixed length, n_episodes = 4, five alternating legs of 0.3 s per side (a leg is at least one call):
  eval    group.evaluate (one acting launch per round) against Evaluator.evaluate(member) for each member of the same group, one
          after the other, member-evaluations/s; the same bar for P >= 8, P = 1 reported without one
  subset  group.sample(members=[0]) against group.sample() of all at P = 64 and 256, us per call (reported, no bar)
--wide measures the layer form of a group (default profiles/bench_dqn_group_wide.json): the reference's dqn_cartpole shape - Mlp[256, 256],
in 4, 2 actions, batch 64, Adam - on full uniform rings of 10 000, same protocol:
  opt    group.opt (11 launches per round whatever P is) against a loop of Agent::opt over the same P agents standalone in their default
         configuration (graph replay included), member-updates/s, the ratio, worst grouped leg over best loop leg, us per group round;
         the bar at P = 8 and 64, P = 1 and 256 reported without one
--sample-full prints one line with the us per call of group.sample of all members at P = 64 (three runs of this commit and of the
parent alternating show that the default path did not move); it writes no file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import border_amd as B  # noqa: E402


def c1(seed, gamma=0.99):
    return B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.MlpConfig(in_dim=4, units=(64, 64), out_dim=2), opt_config=B.OptimizerConfig.Adam(1e-3)),
                       soft_update_interval=1, batch_size=32, tau=0.01, critic_loss="Mse", discount_factor=gamma, device=0, param_seed=seed, train=True)


def ring(seed, rows):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=10000, seed=seed), (4,), np.float32)
    rb.push(*rows)
    return rb


def legs(step, sync, per_step, n_legs, leg_s, chunk):
    """rates (units/s) of n_legs legs of about leg_s seconds: `chunk` steps at a time until the time is up, then a synchronise"""
    out = []
    for _ in range(n_legs):
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < leg_s:
            for _ in range(chunk): step()
            n += chunk
        sync()
        out.append(n * per_step / (time.perf_counter() - t0))
    return out


def measure(a_step, a_sync, b_step, b_sync, per_step, K, n_legs, leg_s):
    """a = the group, b = the sequential loop; alternating legs"""
    for step, sync in ((a_step, a_sync), (b_step, b_sync)):
        for _ in range(50): step()
        sync()
    res = {}
    for name, step, sync in (("group", a_step, a_sync), ("loop", b_step, b_sync)):
        t0 = time.perf_counter()
        for _ in range(K): step()
        sync()
        res[name + "_window"] = K * per_step / (time.perf_counter() - t0)
    la, lb = [], []
    for _ in range(n_legs):
        la += legs(a_step, a_sync, per_step, 1, leg_s, 20)
        lb += legs(b_step, b_sync, per_step, 1, leg_s, 5)
    res["group"] = statistics.median(la); res["group_min_max"] = [min(la), max(la)]
    res["loop"] = statistics.median(lb); res["loop_min_max"] = [min(lb), max(lb)]
    res["ratio"] = res["group"] / res["loop"]
    res["ratio_worst_case"] = min(la) / max(lb)
    res["group_step_us"] = 1e6 * per_step / res["group"]
    return {k: (round(v, 2) if isinstance(v, float) else [round(x, 1) for x in v]) for k, v in res.items()}


def online(args, rows):
    doc = {"bench": "dqn_group_online", "shape": "Mlp[64,64] in 4 A 2, batch 32, ring 5000 / 10000, host rows", "window_steps": args.window,
           "legs": args.legs, "leg_seconds": args.leg_seconds, "unit_push": "member-pushes/s (median of the legs)",
           "unit_iter": "member-iterations/s (median of the legs); one iteration = sample, push, opt of every member",
           "bar": "group_min - loop_max > max(group_max - group_min, loop_max - loop_min)", "push": {}, "iter": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        ga, gb = B.DqnGroup.build([c1(i) for i in range(P)]), B.DqnGroup.build([c1(i) for i in range(P)])
        a_rings, b_rings = [ring(100 + i, rows) for i in range(P)], [ring(100 + i, rows) for i in range(P)]
        pa_rings, pb_rings = [ring(300 + i, rows) for i in range(P)], [ring(300 + i, rows) for i in range(P)]   # the push-only pair
        cols = tuple(np.ascontiguousarray(c[:P]) for c in rows)
        obs = cols[0]
        one = [tuple(c[i:i + 1] for c in cols) for i in range(P)]
        ga.opt(a_rings); gb.opt(b_rings)              # names the buffers; opt() / push() then go on with them
        gp = B.DqnGroup.build([c1(i) for i in range(P)])
        gp.push(*cols, buffers=pa_rings)

        def loop_push():
            for r, t in zip(pb_rings, one): r.push(*t)

        def loop_push_sync():
            for r in pb_rings: r.read_rows(0, 0)      # (synchronises the ring's stream)

        def iter_group():
            ga.sample(obs); ga.push(*cols); ga.opt()

        def iter_loop():
            gb.sample(obs)
            for r, t in zip(b_rings, one): r.push(*t)
            gb.opt()

        for key, m in (("push", measure(lambda: gp.push(*cols), gp.sync, loop_push, loop_push_sync, P, args.window, args.legs, args.leg_seconds)),
                       ("iter", measure(iter_group, ga.sync, iter_loop, gb.sync, P, args.window, args.legs, args.leg_seconds))):
            (g0, g1), (l0, l1) = m["group_min_max"], m["loop_min_max"]
            m["bar_met"] = bool(g0 - l1 > max(g1 - g0, l1 - l0))
            doc[key][str(P)] = m
            print(P, key, m, flush=True)
        for g in (ga, gb, gp): g.close()
        for r in a_rings + b_rings + pa_rings + pb_rings: r.close()
    return doc


class FixedEnv:
    """the evaluator's trivial environment: episodes of `length` steps, a constant row, reward 1"""
    def __init__(self, length=10):
        self.length, self.t, self.row = length, 0, np.zeros(4, np.float32)

    def reset_with_index(self, ix):
        self.t = 0
        return self.row

    def step(self, act):
        self.t += 1
        return self.row, 1.0, self.t == self.length, False


def alternating(a_step, b_step, n_legs, leg_s):
    """calls/s of n_legs legs per side, the sides alternating; a leg runs whole calls until leg_s seconds are up (at least one)"""
    a_step(); b_step()
    out = ([], [])
    for _ in range(n_legs):
        for side, step in enumerate((a_step, b_step)):
            n, t0 = 0, time.perf_counter()
            while n == 0 or time.perf_counter() - t0 < leg_s:
                step(); n += 1
            out[side].append(n / (time.perf_counter() - t0))
    return out


def evaluation(args, rows):
    from border_amd.evaluator import Evaluator
    doc = {"bench": "dqn_group_eval", "shape": "Mlp[64,64] in 4 A 2, members in eval mode, n_episodes 4, episodes of 10 steps, host rows",
           "legs": args.legs, "leg_seconds": args.leg_seconds, "unit_eval": "member-evaluations/s (median of the legs)",
           "unit_subset": "us per call (median of the legs)",
           "bar": "group_min - loop_max > max(group_max - group_min, loop_max - loop_min) for P >= 8; P = 1 is reported without a bar",
           "eval": {}, "subset": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.DqnGroup.build([c1(i) for i in range(P)])
        for m in g.members: m.eval()
        evs = [Evaluator(FixedEnv(), 4, obs_dim=4, act_dim=1, act_dtype=np.int64) for _ in range(P)]
        members = g.members

        def loop_eval():
            for e, m in zip(evs, members): e.evaluate(m)

        la, lb = alternating(lambda: g.evaluate(evs), loop_eval, args.legs, args.leg_seconds)
        la, lb = [x * P for x in la], [x * P for x in lb]
        m = {"group": statistics.median(la), "group_min_max": [min(la), max(la)], "loop": statistics.median(lb), "loop_min_max": [min(lb), max(lb)]}
        m["ratio"] = m["group"] / m["loop"]; m["ratio_worst_case"] = min(la) / max(lb)
        m = {k: (round(v, 2) if isinstance(v, float) else [round(x, 1) for x in v]) for k, v in m.items()}
        (g0, g1), (l0, l1) = m["group_min_max"], m["loop_min_max"]
        m["bar_met"] = bool(g0 - l1 > max(g1 - g0, l1 - l0)) if P >= 8 else None
        doc["eval"][str(P)] = m
        print(P, "eval", m, flush=True)
        if P in (64, 256):
            obs = np.ascontiguousarray(rows[0][:P])
            one, full = alternating(lambda: g.sample(obs, members=[0]), lambda: g.sample(obs), args.legs, args.leg_seconds)
            one, full = [1e6 / x for x in one], [1e6 / x for x in full]
            doc["subset"][str(P)] = {"one_member_us": round(statistics.median(one), 2), "one_member_min_max": [round(min(one), 2), round(max(one), 2)],
                                     "all_members_us": round(statistics.median(full), 2), "all_members_min_max": [round(min(full), 2), round(max(full), 2)]}
            print(P, "subset", doc["subset"][str(P)], flush=True)
        g.close()
    return doc


def sample_full(args, rows):
    P = 64
    g = B.DqnGroup.build([c1(i) for i in range(P)])
    for m in g.members: m.eval()
    obs = np.ascontiguousarray(rows[0][:P])
    for _ in range(200): g.sample(obs)
    us = []
    for _ in range(args.legs):
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < args.leg_seconds:
            for _ in range(20): g.sample(obs)
            n += 20
        us.append(1e6 * (time.perf_counter() - t0) / n)
    g.close()
    print(json.dumps({"sample_full_P64_us": round(statistics.median(us), 2), "min_max": [round(min(us), 2), round(max(us), 2)]}))


def per_ring(seed, rows):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=10000, seed=seed, per_config=B.PerConfig()), (4,), np.float32)
    # FULL rings: a uniform of exactly 0 (word 840 702 of seed 100's stream, update 26 271) descends to the leftmost leaf; in a part-filled
    # ring that leaf was never set, its weight is infinite - in the reference too - and the run ends in NaN priorities
    rb.push(*rows); rb.push(*rows)
    return rb


def prioritized(args, rows):
    doc = {"bench": "dqn_group_per", "shape": "Mlp[64,64] in 4 A 2, batch 32, prioritized rings 10000 / 10000 (PerConfig defaults: alpha 0.6, All), gamma 0, host rows",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds, "unit_opt": "member-updates/s (median of the legs)",
           "unit_iter": "member-iterations/s (median of the legs); one iteration = sample, push, opt of every member",
           "bar": "group_min - loop_max > max(group_max - group_min, loop_max - loop_min); P = 1 is reported without a bar",
           "launches_per_round": "4 in the steady loop (k_per_sample_group, the step, k_per_update_group, k_per_minmax_group), 5 behind a push "
                                 "(k_per_minmax_group first); enqueued by group_round whatever P is",
           "launches_per_push": "3 (k_group_push, k_per_minmax_group, k_per_push_group), 2 when no ring needs its maximum recomputed; whatever P is",
           "opt": {}, "iter": {}}
    # gamma = 0: tens of thousands of bootstrapped updates on random rows can diverge, and a prioritized ring - unlike a uniform one -
    # reports the NaN priority that follows; the work per update is the same
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.DqnGroup.build([c1(i, 0.0) for i in range(P)], prioritized=True)
        g_rings = [per_ring(100 + i, rows) for i in range(P)]
        solo = [B.Dqn.build(c1(i, 0.0)) for i in range(P)]
        s_rings = [per_ring(100 + i, rows) for i in range(P)]
        ga, gb = B.DqnGroup.build([c1(i, 0.0) for i in range(P)], prioritized=True), B.DqnGroup.build([c1(i, 0.0) for i in range(P)], prioritized=True)
        a_rings, b_rings = [per_ring(300 + i, rows) for i in range(P)], [per_ring(300 + i, rows) for i in range(P)]
        cols = tuple(np.ascontiguousarray(c[:P]) for c in rows)
        obs = cols[0]
        one = [tuple(c[i:i + 1] for c in cols) for i in range(P)]
        g.opt(g_rings); ga.opt(a_rings); gb.opt(b_rings)   # names the buffers; opt() / push() then go on with them

        def loop_opt():
            for a, r in zip(solo, s_rings): a.opt(r)

        def loop_sync():
            for a in solo: a.sync()

        def iter_group():
            ga.sample(obs); ga.push(*cols); ga.opt()

        def iter_loop():
            gb.sample(obs)
            for r, t in zip(b_rings, one): r.push(*t)
            gb.opt()

        for key, m in (("opt", measure(g.opt, g.sync, loop_opt, loop_sync, P, args.window, args.legs, args.leg_seconds)),
                       ("iter", measure(iter_group, ga.sync, iter_loop, gb.sync, P, args.window, args.legs, args.leg_seconds))):
            (g0, g1), (l0, l1) = m["group_min_max"], m["loop_min_max"]
            m["bar_met"] = bool(g0 - l1 > max(g1 - g0, l1 - l0)) if P > 1 else None
            doc[key][str(P)] = m
            print(P, key, m, flush=True)
        for x in (g, ga, gb): x.close()
        for a in solo: a.close()
        for r in g_rings + s_rings + a_rings + b_rings: r.close()
    return doc


def wide_cfg(seed):
    return B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.MlpConfig(in_dim=4, units=(256, 256), out_dim=2), opt_config=B.OptimizerConfig.Adam(1e-3)),
                       soft_update_interval=1, batch_size=64, tau=0.01, critic_loss="Mse", discount_factor=0.99, device=0, param_seed=seed, train=True)


def full_ring(seed, rows):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=10000, seed=seed), (4,), np.float32)
    rb.push(*rows); rb.push(*rows)
    return rb


def source_stamp():
    """the hash bench.py ties committed measurements to (kernel sources + the header), so a stale profile can be told from a current one"""
    import bench
    return {"kernel_source_sha16": bench.kernel_source_hash()}


def wide(args, rows):
    doc = {"bench": "dqn_group_wide", "_source": source_stamp(),
           "shape": "dqn_cartpole: Mlp[256,256] in 4 A 2, batch 64, Adam 1e-3, full uniform rings 10000 / 10000", "window_steps": args.window,
           "legs": args.legs, "leg_seconds": args.leg_seconds, "unit_opt": "member-updates/s (median of the legs)",
           "sides": "group.opt of a layer-form DqnGroup against a loop of Agent::opt over the same P agents standalone, default configuration (graph replay included), one process",
           "bar": "at P = 8 and 64: group_min - loop_max > max(group_max - group_min, loop_max - loop_min); P = 1 and 256 are reported without a bar",
           "opt": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.DqnGroup.build([wide_cfg(i) for i in range(P)])
        assert g.form == "layers"
        doc["launches_per_round"] = g.launches_per_round
        g_rings = [full_ring(100 + i, rows) for i in range(P)]
        solo = [B.Dqn.build(wide_cfg(i)) for i in range(P)]
        s_rings = [full_ring(100 + i, rows) for i in range(P)]
        g.opt(g_rings)

        def loop_opt():
            for a, r in zip(solo, s_rings): a.opt(r)

        def loop_sync():
            for a in solo: a.sync()

        m = measure(g.opt, g.sync, loop_opt, loop_sync, P, args.window, args.legs, args.leg_seconds)
        (g0, g1), (l0, l1) = m["group_min_max"], m["loop_min_max"]
        m["bar_met"] = bool(g0 - l1 > max(g1 - g0, l1 - l0)) if P in (8, 64) else None
        doc["opt"][str(P)] = m
        print(P, "opt", m, flush=True)
        g.close()
        for a in solo: a.close()
        for r in g_rings + s_rings: r.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="measure the layer form: dqn_cartpole (Mlp[256, 256], batch 64) group opt against a loop of Agent::opt")
    ap.add_argument("--eval", action="store_true", help="measure the lockstep evaluator against a loop of Evaluator.evaluate, and the subset launch")
    ap.add_argument("--sample-full", action="store_true", help="print the us per call of group.sample of all members at P = 64 and exit")
    ap.add_argument("--per", action="store_true", help="measure prioritized rings under a group: opt and the online iteration")
    ap.add_argument("--online", action="store_true", help="measure group.push and the online iteration instead of opt / sample")
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="default: profiles/bench_dqn_group.json, with --online profiles/bench_dqn_group_online.json, "
                                                "with --per profiles/bench_dqn_group_per.json, "
                                                "with --eval profiles/bench_dqn_group_eval.json, with --wide profiles/bench_dqn_group_wide.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                "bench_dqn_group_wide.json" if args.wide else "bench_dqn_group_eval.json" if args.eval else "bench_dqn_group_per.json" if args.per else "bench_dqn_group_online.json" if args.online else "bench_dqn_group.json")
    rng = np.random.default_rng(0)
    n = 5000
    rows = (rng.standard_normal((n, 4)).astype(np.float32), rng.integers(0, 2, (n, 1)).astype(np.int64),
            rng.standard_normal((n, 4)).astype(np.float32), np.ones(n, np.float32), (rng.random(n) < .1).astype(np.int8), np.zeros(n, np.int8))
    doc = {"bench": "dqn_group", "shape": "Mlp[64,64] in 4 A 2, batch 32, ring 5000 / 10000", "window_steps": args.window, "legs": args.legs,
           "leg_seconds": args.leg_seconds, "unit_opt": "member-updates/s (median of the legs)", "unit_sample": "member-actions/s (median of the legs)",
           "opt": {}, "sample": {}}
    if args.sample_full:
        return sample_full(args, rows)
    if args.wide:
        doc = wide(args, rows)
    elif args.eval:
        doc = evaluation(args, rows)
    elif args.per:
        doc = prioritized(args, rows)
    elif args.online:
        doc = online(args, rows)
    for P in [] if args.online or args.per or args.eval or args.wide else [int(x) for x in args.sizes.split(",")]:
        g = B.DqnGroup.build([c1(i) for i in range(P)])
        g_rings = [ring(100 + i, rows) for i in range(P)]
        solo = [B.Dqn.build(c1(i)) for i in range(P)]
        s_rings = [ring(100 + i, rows) for i in range(P)]
        obs = np.ascontiguousarray(rows[0][:P])       # one [P, in_dim] array: the group's rows by address arithmetic
        obs1 = [obs[i:i + 1] for i in range(P)]
        g.opt(g_rings)                                # names the buffers; opt() then steps on them again

        def loop_opt():
            for a, r in zip(solo, s_rings): a.opt(r)

        def loop_sync():
            for a in solo: a.sync()

        def loop_sample():
            for a, o in zip(solo, obs1): a.sample(o)

        doc["opt"][str(P)] = measure(g.opt, g.sync, loop_opt, loop_sync, P, args.window, args.legs, args.leg_seconds)
        doc["sample"][str(P)] = measure(lambda: g.sample(obs), lambda: None, loop_sample, lambda: None, P, args.window, args.legs, args.leg_seconds)
        print(P, "opt", doc["opt"][str(P)], flush=True)
        print(P, "sample", doc["sample"][str(P)], flush=True)
        g.close()
        for a in solo: a.close()
        for r in g_rings + s_rings: r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.abspath(args.out)}))


if __name__ == "__main__":
    main()
