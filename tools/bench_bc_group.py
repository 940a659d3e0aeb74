"""Aggregate member-updates/s of a BcGroup (2L + 2 launches per round whatever P is) against a loop of Agent::opt over the same P agents
standalone, in one process, at the bc_pen shape: obs 45, act 24, Mlp[256, 256] with a Tanh output, B = 256, AdamW, the default kernel
form (the MFMA head) - P in {1, 8, 64}.  The data of both sides are VIEWS of one ring of 100 000 rows (SimpleReplayBuffer.view): P index
streams over one copy of the rows.

Protocol (tools/bench_dqn_group.py --wide): warm-up, one window of K = 300 rounds per side, then five legs of 0.3 s per side, the two
sides alternating; the figure is the median of the legs, the spread their min / max.  The bar: at P = 8 the group's worst leg lies
above the loop's best leg; P = 1 and P = 64 are reported without one.  Also reported: us per group round, and the HBM held by the
rows of P views against P rings of their own.  Writes one JSON document (default profiles/bench_bc_group.json).

--act   ONE group acting call (bdr_bc_group_sample) of one float64 row per member with a normaliser against a loop of
        bdr_agent_sample_raw over the same P agents standalone, each on its faster act path (both paths are measured in the same run
        and the faster one is the loop's): member-actions/s.  Both sides call the C ABI on arrays prepared ahead.
--eval  BcGroup.evaluate against Evaluator.evaluate member after member, 4 episodes of 10 steps per member on float64 rows with a
        normaliser (a scripted environment in Python on both sides): member-evaluations/s.
Both follow the protocol above with a short warm-up (the calls are synchronous) and the same bar at P = 8, and write
profiles/bench_bc_group_act.json / profiles/bench_bc_group_eval.json."""
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
from bench_dqn_group import legs, measure  # noqa: E402
from border_amd import _lib  # noqa: E402

OBS, ACT, UNITS, BATCH, ROWS = 45, 24, (256, 256), 256, 100_000


def config(i):
    opt = B.OptimizerConfig.AdamW(1e-3 * (1 + 0.01 * i))
    return B.BcConfig(obs_dim=OBS, act_dim=ACT, policy_model_config=B.BcModelConfig(B.CandleMlpConfig(UNITS, "Tanh"), opt), batch_size=BATCH,
                      action_type="Continuous", device=0, seed=i)


def ring_bytes(capacity):
    """capacity x record stride (include/border_amd.h: obs | next_obs | act | reward, flags; 16-byte aligned sections)"""
    up = lambda x, a: (x + a - 1) // a * a
    next_off = up(OBS * 4, 16)
    act_off = up(next_off + OBS * 4, 16)
    raw = up(act_off + ACT * 4, 8) + 8
    return capacity * up(raw, 128 if raw >= 1024 else 16)


def measure_sync(a_step, b_step, per_step, warm, n_legs, leg_s, chunk):
    """bench_dqn_group.measure for synchronous calls: a = the group, b = the loop; warm-up, then alternating legs"""
    nothing = lambda: None
    for step in (a_step, b_step):
        for _ in range(warm): step()
    la, lb = [], []
    for _ in range(n_legs):
        la += legs(a_step, nothing, per_step, 1, leg_s, chunk)
        lb += legs(b_step, nothing, per_step, 1, leg_s, chunk)
    res = {"group": statistics.median(la), "group_min_max": [min(la), max(la)], "loop": statistics.median(lb), "loop_min_max": [min(lb), max(lb)]}
    res["ratio"] = res["group"] / res["loop"]
    res["ratio_worst_case"] = min(la) / max(lb)
    res["group_call_us"] = 1e6 * per_step / res["group"]
    res["loop_call_us"] = 1e6 / res["loop"]
    return {k: (round(v, 2) if isinstance(v, float) else [round(x, 1) for x in v]) for k, v in res.items()}


def normaliser():
    rng = np.random.default_rng(9)
    return B.ObsNormalizer(OBS, 0).set(rng.standard_normal(OBS).astype(np.float32), rng.uniform(0.5, 2.0, OBS).astype(np.float32))


def act(args):
    doc = {"bench": "bc_group_act", "shape": "bc_pen: obs 45, act 24, Mlp[256,256] Tanh; one float64 row per member, a normaliser",
           "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-actions/s (median of the legs); loop = bdr_agent_sample_raw of the same P agents standalone, each on its faster act path",
           "bar": "at P = 8: group_min > loop_max", "act": {}}
    L, nz = _lib.lib(), normaliser()
    rng = np.random.default_rng(1)
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.BcGroup.build([config(i) for i in range(P)])
        solo = [B.Bc.build(config(i)) for i in range(P)]
        rows = [rng.standard_normal((1, OBS)) for _ in range(P)]
        outs_g, outs_l = [np.empty((1, ACT), np.float32) for _ in range(P)], [np.empty((1, ACT), np.float32) for _ in range(P)]
        rp, gp, cp = (C.c_void_p * P)(*[r.ctypes.data for r in rows]), (C.c_void_p * P)(*[o.ctypes.data for o in outs_g]), (C.c_int32 * P)(*[_lib.BDR_DTYPE_F64] * P)
        npp = (C.c_void_p * P)(*[nz.handle] * P)
        each = [(a.handle, C.c_void_p(r.ctypes.data), C.c_void_p(o.ctypes.data)) for a, r, o in zip(solo, rows, outs_l)]

        def group_call():
            _lib.check(L.bdr_bc_group_sample(g.handle, npp, 1, rp, cp, gp))

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


class PenLikeEnv:
    """4 episodes of 10 steps: float64 observation rows that are a fixed function of (episode, step); the reward is the action's sum"""
    def __init__(self, m):
        self.m, self.ix, self.t = m, 0, 0

    def obs(self):
        return np.sin(0.37 * np.arange(OBS, dtype=np.float64) + self.m + 3.0 * self.ix + 0.5 * self.t)

    def reset_with_index(self, ix):
        self.ix, self.t = ix, 0
        return self.obs()

    def step(self, a):
        self.t += 1
        return self.obs(), float(a.sum()), self.t == 10, False


def evaluate(args):
    doc = {"bench": "bc_group_eval", "shape": "bc_pen: obs 45, act 24, Mlp[256,256] Tanh; 4 episodes of 10 steps per member, float64 rows, a normaliser",
           "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-evaluations/s (median of the legs); loop = Evaluator.evaluate of the same P agents standalone, one after the other, each on its faster act path",
           "bar": "at P = 8: group_min > loop_max", "eval": {}}
    nz = normaliser()
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.BcGroup.build([config(i) for i in range(P)])
        solo = [B.Bc.build(config(i)) for i in range(P)]
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
    ap.add_argument("--eval", action="store_true", help="BcGroup.evaluate against Evaluator.evaluate member after member")
    ap.add_argument("--warm", type=int, default=50, help="warm-up calls per side of --act")
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_bc_group.json"))
    args = ap.parse_args()
    if args.act or args.eval:
        for on, run, name in ((args.act, act, "bench_bc_group_act.json"), (args.eval, evaluate, "bench_bc_group_eval.json")):
            if not on: continue
            out = os.path.join(os.path.dirname(os.path.abspath(args.out)), name)
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
                   rng.standard_normal((n, OBS)).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.int8), np.zeros(n, np.int8))
    doc = {"bench": "bc_group", "shape": "bc_pen: obs 45, act 24, Mlp[256,256] Tanh, B 256, AdamW, default kernel form; views of one ring of 100000 rows",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-updates/s (median of the legs); loop = bdr_agent_opt of the same P agents standalone, one after the other",
           "bar": "at P = 8: group_min > loop_max", "opt": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.BcGroup.build([config(i) for i in range(P)])
        solo = [B.Bc.build(config(i)) for i in range(P)]
        gv, sv = [owner.view(100 + i) for i in range(P)], [owner.view(100 + i) for i in range(P)]
        g.opt(gv)   # names the buffers; opt() then goes on with them

        def loop():
            for a, v in zip(solo, sv): a.opt(v)

        def loop_sync():
            for a in solo: a.sync()

        m = measure(g.opt, g.sync, loop, loop_sync, P, args.window, args.legs, args.leg_seconds)
        m["launches_per_round"] = g.launches_per_round
        m["hbm_rows_P_views_MB"] = round(ring_bytes(ROWS) / 1e6, 1)
        m["hbm_rows_P_rings_MB"] = round(P * ring_bytes(ROWS) / 1e6, 1)
        if P == 8:
            m["bar_met"] = bool(m["group_min_max"][0] > m["loop_min_max"][1])
        doc["opt"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
        for v in gv + sv: v.close()
    owner.close()
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(args.out))


if __name__ == "__main__":
    main()
