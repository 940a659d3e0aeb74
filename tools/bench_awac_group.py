"""Aggregate member-updates/s of an AwacGroup (3 (Lp + Lq) + 8 = 32 launches per round whatever P is) against a loop of Agent::opt
(bdr_agent_opt) over the same P agents standalone, in one process, at the pen shape: obs 45, act 24, critic and actor
Mlp[256, 256, 256], two critics, B = 256, Adam, train mode (every update draws act_ and next_act from the member's noise stream) - P in
{1, 8, 64}.  The data of both sides are VIEWS of one ring of 100 000 rows (SimpleReplayBuffer.view): P index streams over one copy of
the rows.

Protocol (tools/bench_dqn_group.py --wide, tools/bench_iql_group.py): warm-up, one window of K = 300 rounds per side, then five legs of
0.3 s per side, the two sides alternating; the figure is the median of the legs, the spread their min / max.  The bar: at P = 8 the
group's worst leg lies above the loop's best leg; P = 1 (the group's cost against the agent alone) and P = 64 are reported without
one.  Writes one JSON document (default profiles/bench_awac_group.json).

--act   ONE group acting call (bdr_awac_group_sample) of one float64 row per member with a normaliser against a loop of
        bdr_agent_sample_raw over the same P agents standalone, each on its faster act path (both paths are measured in the same run
        and the faster one is the loop's): member-actions/s.  Both sides call the C ABI on arrays prepared ahead; the agents are in
        eval mode, so the two sides are also checked to give the same bits.
--eval  AwacGroup.evaluate against Evaluator.evaluate member after member, 4 episodes of 10 steps per member on float64 rows with a
        normaliser (a scripted environment in Python on both sides): member-evaluations/s.
Both follow tools/bench_bc_group.py's protocol for synchronous calls and the same bar at P = 8, and write
profiles/bench_awac_group_act.json / profiles/bench_awac_group_eval.json.
--online  the online iteration group sample -> push -> group opt with the grouped push (AwacGroup.push, one launch) against the same
        iteration with P rb.push calls in the middle, and the push alone (tools/bench_cgroup_online.py has the protocol and the bar);
        writes profiles/bench_awac_group_online.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_amd as B  # noqa: E402
from bench_bc_group import PenLikeEnv, measure_sync, normaliser  # noqa: E402  (the same obs 45 / act 24 rows and protocol)
from bench_dqn_group import legs, measure  # noqa: E402
from border_amd import _lib  # noqa: E402
from border_amd.iql import CandleMlpConfig, GaussianActorConfig, MultiCriticConfig  # noqa: E402

OBS, ACT, UNITS, BATCH, ROWS = 45, 24, (256, 256, 256), 256, 100_000


def config(i, train=False):
    """a sweep over temperature, weight clip, advantage form and seed"""
    opt = lambda: B.OptimizerConfig.Adam(3e-4)
    return B.AwacConfig(obs_dim=OBS, act_dim=ACT, critic_config=MultiCriticConfig(2, CandleMlpConfig(UNITS), opt(), 0.005),
                        actor_config=GaussianActorConfig(CandleMlpConfig(UNITS), opt()), inv_lambda=(0.5, 3.0, 10.0)[i % 3],
                        exp_adv_max=(20.0, 100.0)[i % 2], adv_softmax=i % 5 == 4, batch_size=BATCH, train=train, seed=i, device=0)


SHAPE = "pen: obs 45, act 24, actor Mlp[256,256,256]"


def act(args):
    doc = {"bench": "awac_group_act", "shape": SHAPE + "; one float64 row per member, a normaliser, eval mode",
           "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-actions/s (median of the legs); loop = bdr_agent_sample_raw of the same P agents standalone, each on its faster act path",
           "bar": "at P = 8: group_min > loop_max", "act": {}}
    L, nz = _lib.lib(), normaliser()
    rng = np.random.default_rng(1)
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.AwacGroup.build([config(i) for i in range(P)])
        solo = [B.Awac.build(config(i)) for i in range(P)]
        rows = [rng.standard_normal((1, OBS)) for _ in range(P)]
        outs_g, outs_l = [np.empty((1, ACT), np.float32) for _ in range(P)], [np.empty((1, ACT), np.float32) for _ in range(P)]
        rp, gp, cp = (C.c_void_p * P)(*[r.ctypes.data for r in rows]), (C.c_void_p * P)(*[o.ctypes.data for o in outs_g]), (C.c_int32 * P)(*[_lib.BDR_DTYPE_F64] * P)
        npp = (C.c_void_p * P)(*[nz.handle] * P)
        each = [(a.handle, C.c_void_p(r.ctypes.data), C.c_void_p(o.ctypes.data)) for a, r, o in zip(solo, rows, outs_l)]

        def group_call():
            _lib.check(L.bdr_awac_group_sample(g.handle, npp, 1, rp, cp, gp))

        def loop_call():
            for h, r, o in each: _lib.check(L.bdr_agent_sample_raw(h, nz.handle, 1, r, _lib.BDR_DTYPE_F64, 0, 0, o, None))
        # the loop's act path: whichever of the two is faster for this call on this machine, measured here
        paths = {}
        for path in ("layers", "fused"):
            for a in solo: a.set_act_path(path)
            for _ in range(args.warm): loop_call()
            paths[path] = statistics.median(legs(loop_call, lambda: None, P, 3, args.leg_seconds / 3, 5))
        best = max(paths, key=paths.get)
        for a in solo: a.set_act_path(best)
        group_call(); loop_call()
        assert all(np.array_equal(x, y) for x, y in zip(outs_g, outs_l)), "the group's actions are not the members' own"
        m = measure_sync(group_call, loop_call, P, args.warm, args.legs, args.leg_seconds, 5)
        m["loop_act_path"] = best
        m["loop_paths_member_actions_per_s"] = {k: round(v, 1) for k, v in paths.items()}
        if P == 8:
            m["bar_met"] = bool(m["group_min_max"][0] > m["loop_min_max"][1])
        doc["act"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
    nz.close()
    return doc


def evaluate(args):
    doc = {"bench": "awac_group_eval", "shape": SHAPE + "; 4 episodes of 10 steps per member, float64 rows, a normaliser, eval mode",
           "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-evaluations/s (median of the legs); loop = Evaluator.evaluate of the same P agents standalone, one after the other, each on its faster act path",
           "bar": "at P = 8: group_min > loop_max", "eval": {}}
    nz = normaliser()
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.AwacGroup.build([config(i) for i in range(P)])
        solo = [B.Awac.build(config(i)) for i in range(P)]
        mk = lambda: [B.Evaluator(PenLikeEnv(i), 4, obs_norm=nz, obs_dtype=np.float64, act_dim=ACT, act_dtype=np.float32) for i in range(P)]
        ge, le = mk(), mk()

        def group_call():
            return g.evaluate(ge)

        def loop_call():
            return [e.evaluate(a) for e, a in zip(le, solo)]
        paths = {}
        for path in ("layers", "fused"):
            for a in solo: a.set_act_path(path)
            for _ in range(2): loop_call()
            paths[path] = statistics.median(legs(loop_call, lambda: None, P, 3, args.leg_seconds / 3, 1))
        best = max(paths, key=paths.get)
        for a in solo: a.set_act_path(best)
        assert [np.float32(x.score).tobytes() for x in group_call()] == [np.float32(x.score).tobytes() for x in loop_call()], "the group's scores are not the members' own"
        m = measure_sync(group_call, loop_call, P, 2, args.legs, args.leg_seconds, 1)
        m["loop_act_path"] = best
        m["loop_paths_member_evaluations_per_s"] = {k: round(v, 1) for k, v in paths.items()}
        if P == 8:
            m["bar_met"] = bool(m["group_min_max"][0] > m["loop_min_max"][1])
        doc["eval"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
    nz.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--act", action="store_true", help="the group acting call against a loop of bdr_agent_sample_raw")
    ap.add_argument("--eval", action="store_true", help="AwacGroup.evaluate against Evaluator.evaluate member after member")
    ap.add_argument("--online", action="store_true", help="the online iteration with the grouped push against P rb.push calls, and the push alone")
    ap.add_argument("--warm", type=int, default=50, help="warm-up calls per side of --act")
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_awac_group.json"))
    args = ap.parse_args()
    if args.online:
        from bench_cgroup_online import online
        out = os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench_awac_group_online.json")
        doc = online(args, "awac_group_online", SHAPE, "bdr_awac_group", B.AwacGroup, B.Awac, config, OBS, ACT)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", os.path.relpath(out))
        return
    if args.act or args.eval:
        for on, run, name in ((args.act, act, "bench_awac_group_act.json"), (args.eval, evaluate, "bench_awac_group_eval.json")):
            if not on: continue
            out = os.path.join(os.path.dirname(os.path.abspath(args.out)), name)
            os.makedirs(os.path.dirname(out), exist_ok=True)
            with open(out, "w") as f:
                json.dump(run(args), f, indent=1)
                f.write("\n")
            print("wrote", os.path.relpath(out))
        return
    rng = np.random.default_rng(0)
    owner = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=ROWS, seed=1), (OBS,), np.float32, (ACT,), np.float32, device=0)
    for _ in range(ROWS // 10_000):
        n = 10_000
        owner.push(rng.standard_normal((n, OBS)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ACT)).astype(np.float32),
                   rng.standard_normal((n, OBS)).astype(np.float32), rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.01).astype(np.int8),
                   np.zeros(n, np.int8))
    doc = {"bench": "awac_group", "shape": "pen: obs 45, act 24, critic / actor Mlp[256,256,256], 2 critics, B 256, Adam, train mode; views of one ring of 100000 rows",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-updates/s (median of the legs); loop = bdr_agent_opt of the same P agents standalone, one after the other",
           "bar": "at P = 8: group_min > loop_max", "opt": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.AwacGroup.build([config(i, True) for i in range(P)])
        solo = [B.Awac.build(config(i, True)) for i in range(P)]
        gv, sv = [owner.view(100 + i) for i in range(P)], [owner.view(100 + i) for i in range(P)]
        g.opt(gv)   # names the buffers; opt() then goes on with them

        def loop():
            for a, v in zip(solo, sv): a.opt(v)

        def loop_sync():
            for a in solo: a.sync()

        m = measure(g.opt, g.sync, loop, loop_sync, P, args.window, args.legs, args.leg_seconds)
        m["launches_per_round"] = g.launches_per_round
        if P == 8:
            m["bar_met"] = bool(m["group_min_max"][0] > m["loop_min_max"][1])
        doc["opt"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
        for v in gv + sv: v.close()
    owner.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(args.out))


if __name__ == "__main__":
    main()
