"""Aggregate member-updates/s of a CandleDqnGroup (2 L + 4 = 10 launches per round whatever P is) against a loop of Agent::opt
(bdr_agent_opt) over the same P agents standalone, in one process, at the dqn_cartpole shape: obs 4, 2 actions, Mlp[256, 256], B = 64,
AdamW, Mse - P in {1, 8, 64}.  The data of both sides are VIEWS of one ring of 100 000 rows (SimpleReplayBuffer.view): P index streams
over one copy of the rows.

Protocol (tools/bench_dqn_group.py --wide, tools/bench_candle_sac_group.py): warm-up, one window of K = 300 rounds per side, then five
legs of 0.3 s per side, the two sides alternating, a synchronise per leg; the figure is the median of the legs, the spread their min /
max.  The bar, at P = 8 and P = 64: the group's worst leg is not below the loop's best leg; P = 1 (the cost of a group of one against
the agent alone) is reported without one.  Writes one JSON document (default profiles/bench_candle_dqn_group.json).

--act     ONE group acting call (bdr_candle_dqn_group_sample) of one float32 row per member, epsilon-greedy in train mode, against a
          loop of bdr_agent_sample_raw over the same P agents standalone, each on its faster act path (both paths are measured in the
          same run and the faster one is the loop's): member-actions/s.  Both sides call the C ABI on arrays prepared ahead and are
          checked to give the same actions.  Writes profiles/bench_candle_dqn_group_act.json.
--eval    CandleDqnGroup.evaluate against Evaluator.evaluate member after member, 4 episodes of 10 steps per member (a scripted
          environment in Python on both sides): member-evaluations/s.  Writes profiles/bench_candle_dqn_group_eval.json.
--online  the online iteration: group sample -> grouped push -> group opt (3 calls, 12 launches) against the loop an online sweep
          over P standalone agents runs - bdr_agent_sample_raw, bdr_replay_push and bdr_agent_opt per member -, and the push alone;
          every member has a ring of its own (capacity 10 000, 5 000 rows to begin with).  Writes
          profiles/bench_candle_dqn_group_online.json."""
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
from bench_bc_group import measure_sync  # noqa: E402
from bench_dqn_group import legs, measure  # noqa: E402
from border_amd import _lib  # noqa: E402
from border_amd.iql import CandleMlpConfig  # noqa: E402

OBS, ACTIONS, UNITS, BATCH, ROWS = 4, 2, (256, 256), 64, 100_000
RING, FILLED = 10_000, 5_000
SHAPE = "dqn_cartpole: obs 4, 2 actions, Mlp[256,256], B 64, AdamW, Mse"


def config(i, train=False):
    """a sweep over seed, learning rate, discount and the soft-update interval"""
    return B.CandleDqnConfig(obs_dim=OBS, n_actions=ACTIONS,
                             model_config=B.CandleDqnModelConfig(CandleMlpConfig(UNITS), B.OptimizerConfig.AdamW((1e-3, 3e-4)[i % 2])),
                             soft_update_interval=(1, 2, 4)[i % 3], batch_size=BATCH, discount_factor=(0.99, 0.98)[i % 2], tau=0.005, train=train,
                             explorer=B.EpsilonGreedy(eps_start=1.0, eps_final=0.02, final_step=10_000), explorer_seed=42 + i, critic_loss="Mse",
                             seed=i, device=0)


def rows(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, OBS)).astype(np.float32), rng.integers(0, ACTIONS, (n, 1)).astype(np.int64), rng.standard_normal((n, OBS)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))


def ring(capacity, seed, fill=None):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed), (OBS,), np.float32, (1,), np.int64, device=0)
    if fill is not None:
        rb.push(*fill)
    return rb


def bar(m, P):
    if P > 1:
        m["bar_met"] = bool(m["group_min_max"][0] >= m["loop_min_max"][1])
    return m


def faster_path(solo, loop_call, per_step, warm, leg_seconds, chunk):
    """the loop's act path: whichever of the two is faster for this call on this machine, measured here"""
    paths = {}
    for path in ("layers", "fused"):
        for a in solo: a.set_act_path(path)
        for _ in range(warm): loop_call()
        paths[path] = statistics.median(legs(loop_call, lambda: None, per_step, 3, leg_seconds / 3, chunk))
    best = max(paths, key=paths.get)
    for a in solo: a.set_act_path(best)
    return best, {k: round(v, 1) for k, v in paths.items()}


def act(args):
    doc = {"bench": "candle_dqn_group_act", "shape": SHAPE + "; one float32 row per member, epsilon-greedy, train mode",
           "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-actions/s (median of the legs); loop = bdr_agent_sample_raw of the same P agents standalone, each on its faster act path",
           "bar": "at P = 8 and P = 64: group_min >= loop_max", "act": {}}
    L = _lib.lib()
    rng = np.random.default_rng(1)
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.CandleDqnGroup.build([config(i, True) for i in range(P)])
        solo = [B.CandleDqn.build(config(i, True)) for i in range(P)]
        obs = [rng.standard_normal((1, OBS)).astype(np.float32) for _ in range(P)]
        out_g, out_l = np.zeros(P, np.int64), np.zeros(P, np.int64)
        rp, cp = (C.c_void_p * P)(*[r.ctypes.data for r in obs]), (C.c_int32 * P)(*[_lib.BDR_DTYPE_F32] * P)
        gp = (C.c_void_p * P)(*[out_g[i:i + 1].ctypes.data for i in range(P)])
        each = [(a.handle, C.c_void_p(r.ctypes.data), C.c_void_p(out_l[i:i + 1].ctypes.data)) for i, (a, r) in enumerate(zip(solo, obs))]

        def group_call():
            _lib.check(L.bdr_candle_dqn_group_sample(g.handle, None, 1, rp, cp, gp))

        def loop_call():
            for h, r, o in each: _lib.check(L.bdr_agent_sample_raw(h, None, 1, r, _lib.BDR_DTYPE_F32, 0, 0, None, o))
        best, paths = faster_path(solo, loop_call, P, args.warm, args.leg_seconds, 5)
        # the same point of every explorer stream on both sides, then the same actions
        for a in list(g.members) + solo: a.set_explorer(B.EpsilonGreedy(eps_start=1.0, eps_final=0.02, final_step=10_000), seed=7)
        for _ in range(20):
            group_call(); loop_call()
            assert (out_g == out_l).all(), "the group's actions are not the members' own"
        m = bar(measure_sync(group_call, loop_call, P, args.warm, args.legs, args.leg_seconds, 5), P)
        m["loop_act_path"], m["loop_paths_member_actions_per_s"] = best, paths
        doc["act"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
    return doc


class ScriptedEnv:
    """episodes of 10 steps; observations and rewards depend on the action taken"""
    def __init__(self, seed):
        self.seed, self.rng, self.left = seed, None, 0

    def reset_with_index(self, ix):
        self.rng = np.random.default_rng([self.seed, ix])
        self.left = 10
        return self.rng.standard_normal(OBS).astype(np.float32)

    def step(self, act):
        a = int(np.asarray(act).reshape(-1)[0])
        self.left -= 1
        return (self.rng.standard_normal(OBS) + 0.25 * a).astype(np.float32), 1.0 + 0.5 * a, self.left == 0, False


def evaluate(args):
    doc = {"bench": "candle_dqn_group_eval", "shape": SHAPE + "; 4 episodes of 10 steps per member, float32 rows, eval mode",
           "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-evaluations/s (median of the legs); loop = Evaluator.evaluate of the same P agents standalone, one after the other, each on its faster act path",
           "bar": "at P = 8 and P = 64: group_min >= loop_max", "eval": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.CandleDqnGroup.build([config(i) for i in range(P)])
        solo = [B.CandleDqn.build(config(i)) for i in range(P)]
        mk = lambda: [B.Evaluator(ScriptedEnv(i), 4, obs_dim=OBS, act_dim=1, act_dtype=np.int64) for i in range(P)]
        ge, le = mk(), mk()

        def group_call():
            return g.evaluate(ge)

        def loop_call():
            return [e.evaluate(a) for e, a in zip(le, solo)]
        best, paths = faster_path(solo, loop_call, P, 2, args.leg_seconds, 1)
        # (eval mode still draws - one action in a hundred is random: the same point of every explorer stream on both sides)
        for a in list(g.members) + solo: a.set_explorer(B.EpsilonGreedy(eps_start=1.0, eps_final=0.02, final_step=10_000), seed=7)
        assert [np.float32(x.score).tobytes() for x in group_call()] == [np.float32(x.score).tobytes() for x in loop_call()], "the group's scores are not the members' own"
        m = bar(measure_sync(group_call, loop_call, P, 2, args.legs, args.leg_seconds, 1), P)
        m["loop_act_path"], m["loop_paths_member_evaluations_per_s"] = best, paths
        doc["eval"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
    return doc


def online(args):
    doc = {"bench": "candle_dqn_group_online", "shape": SHAPE + f"; train mode, epsilon-greedy, one ring of {RING} rows per member ({FILLED} to begin with), host f32 rows, C calls on prepared arrays",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds, "unit_push": "member-pushes/s (median of the legs)",
           "unit_iter": "member-iterations/s (median of the legs); group: ONE sample, ONE push, ONE opt for all members; loop: bdr_agent_sample_raw (the faster act path), "
                        "bdr_replay_push and bdr_agent_opt of every member, standalone agents",
           "bar": "at P = 8 and P = 64: group_min >= loop_max", "push": {}, "iter": {}}
    L = _lib.lib()
    vp = C.c_void_p
    fill = rows(FILLED, 0)
    for P in [int(x) for x in args.sizes.split(",")]:
        g, gp = (B.CandleDqnGroup.build([config(i, True) for i in range(P)]) for _ in range(2))
        solo = [B.CandleDqn.build(config(i, True)) for i in range(P)]
        g_rings, s_rings, pa_rings, pb_rings = ([ring(RING, 100 + i, fill) for i in range(P)] for _ in range(4))
        cols = rows(P, 1)
        ptrs = [(vp * P)(*[c[i:i + 1].ctypes.data for i in range(P)]) for c in cols]   # per field: one row per member
        each = [tuple(vp(c[i:i + 1].ctypes.data) for c in cols) for i in range(P)]
        codes = (C.c_int32 * P)(*[_lib.BDR_DTYPE_F32] * P)
        outs, outs_l = np.zeros(P, np.int64), np.zeros(P, np.int64)
        out_ptrs = (vp * P)(*[outs[i:i + 1].ctypes.data for i in range(P)])
        hs = {id(rs): (vp * P)(*[r.handle for r in rs]) for rs in (g_rings, pa_rings)}
        g.opt(g_rings)

        def group_push(grp, rs):
            _lib.check(L.bdr_candle_dqn_group_push(grp.handle, hs[id(rs)], 1, ptrs[0], ptrs[2], codes, ptrs[1], ptrs[3], ptrs[4], ptrs[5]))

        def loop_push(rs):
            for r, (o, a, x, rew, t, u) in zip(rs, each): _lib.check(L.bdr_replay_push(r.handle, 1, o, a, x, rew, t, u))

        def iter_group():
            _lib.check(L.bdr_candle_dqn_group_sample(g.handle, None, 1, ptrs[0], codes, out_ptrs))
            group_push(g, g_rings)
            _lib.check(L.bdr_candle_dqn_group_opt(g.handle, hs[id(g_rings)]))

        def sample_loop():
            for i, a in enumerate(solo): _lib.check(L.bdr_agent_sample_raw(a.handle, None, 1, each[i][0], _lib.BDR_DTYPE_F32, 0, 0, None, vp(outs_l[i:i + 1].ctypes.data)))

        def iter_loop():
            for i, (a, r) in enumerate(zip(solo, s_rings)):
                o, ac, x, rew, t, u = each[i]
                _lib.check(L.bdr_agent_sample_raw(a.handle, None, 1, o, _lib.BDR_DTYPE_F32, 0, 0, None, vp(outs_l[i:i + 1].ctypes.data)))
                _lib.check(L.bdr_replay_push(r.handle, 1, o, ac, x, rew, t, u))
                _lib.check(L.bdr_agent_opt(a.handle, r.handle))

        def loop_sync():
            for a in solo: a.sync()

        def loop_push_sync():
            for r in pb_rings: r.read_rows(0, 0)      # (synchronises the ring's stream)
        best, paths = faster_path(solo, sample_loop, P, args.warm, args.leg_seconds, 5)
        group_push(gp, pa_rings)
        for key, m in (("push", measure(lambda: group_push(gp, pa_rings), gp.sync, lambda: loop_push(pb_rings), loop_push_sync, P, args.window, args.legs, args.leg_seconds)),
                       ("iter", measure(iter_group, g.sync, iter_loop, loop_sync, P, args.window, args.legs, args.leg_seconds))):
            bar(m, P)
            if key == "iter":
                m["loop_act_path"] = best
            doc[key][str(P)] = m
            print(P, key, m, flush=True)
        for x in (g, gp): x.close()
        for a in solo: a.close()
        for r in g_rings + s_rings + pa_rings + pb_rings: r.close()
    return doc


def rounds(args):
    rng = np.random.default_rng(0)
    owner = ring(ROWS, 1)
    for _ in range(ROWS // 10_000):
        n = 10_000
        owner.push(rng.standard_normal((n, OBS)).astype(np.float32), rng.integers(0, ACTIONS, (n, 1)).astype(np.int64), rng.standard_normal((n, OBS)).astype(np.float32),
                   rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))
    doc = {"bench": "candle_dqn_group", "shape": SHAPE + "; views of one ring of 100000 rows",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-updates/s (median of the legs); loop = bdr_agent_opt of the same P agents standalone, one after the other",
           "bar": "at P = 8 and P = 64: group_min >= loop_max", "opt": {}}
    for P in [int(x) for x in args.sizes.split(",")]:
        g = B.CandleDqnGroup.build([config(i, True) for i in range(P)])
        solo = [B.CandleDqn.build(config(i, True)) for i in range(P)]
        gv, sv = [owner.view(100 + i) for i in range(P)], [owner.view(100 + i) for i in range(P)]
        g.opt(gv)   # names the buffers; opt() then goes on with them

        def loop():
            for a, v in zip(solo, sv): a.opt(v)

        def loop_sync():
            for a in solo: a.sync()

        m = bar(measure(g.opt, g.sync, loop, loop_sync, P, args.window, args.legs, args.leg_seconds), P)
        m["launches_per_round"] = g.launches_per_round
        doc["opt"][str(P)] = m
        print(P, m, flush=True)
        g.close()
        for a in solo: a.close()
        for v in gv + sv: v.close()
    owner.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--act", action="store_true", help="the group acting call against a loop of bdr_agent_sample_raw")
    ap.add_argument("--eval", action="store_true", help="CandleDqnGroup.evaluate against Evaluator.evaluate member after member")
    ap.add_argument("--online", action="store_true", help="the online iteration against the loop over standalone agents, and the push alone")
    ap.add_argument("--warm", type=int, default=50, help="warm-up calls per side of --act")
    ap.add_argument("--sizes", default="1,8,64")
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_candle_dqn_group.json"))
    args = ap.parse_args()
    runs = [(on, run, name) for on, run, name in ((args.act, act, "bench_candle_dqn_group_act.json"), (args.eval, evaluate, "bench_candle_dqn_group_eval.json"),
                                                  (args.online, online, "bench_candle_dqn_group_online.json")) if on]
    if not runs:
        runs = [(True, rounds, os.path.basename(args.out))]
    for _on, run, name in runs:
        out = os.path.join(os.path.dirname(os.path.abspath(args.out)), name)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        doc = run(args)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", os.path.relpath(out))


if __name__ == "__main__":
    main()
