"""The online side of a continuous-action group (tools/bench_candle_sac_group.py --online, tools/bench_awac_group.py --online), in the
form of tools/bench_dqn_group.py --online, at the pen shape with P in {1, 8, 64}; every member has a ring of its own (capacity 10 000,
5 000 rows to begin with) and all calls go to the C ABI on arrays prepared ahead:
  iter   one online iteration group sample -> push -> group opt: the grouped push (ONE launch) against the same iteration in the same
         process with the P bdr_replay_push calls in the middle - what an online loop over a group had to be before the grouped
         push -, member-iterations/s
  push   the push alone: one grouped push of one transition per member against a loop of bdr_replay_push, member-pushes/s
  lone   at P = 1 also the lone agent's iteration (bdr_agent_sample_raw -> bdr_replay_push -> bdr_agent_opt): the cost of a group of one
Protocol (bench_dqn_group.measure): warm-up, one window of K = 300 steps per side, then five legs of 0.3 s per side, the two sides
alternating; the figure is the median of the legs, the spread their min / max.  The bar, at P = 8 and P = 64: the worst grouped leg is
not below the best loop leg."""
import ctypes as C

import numpy as np

import border_amd as B
from bench_dqn_group import measure
from border_amd import _lib

RING, FILLED = 10_000, 5_000


def rows(obs, act, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, obs)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, act)).astype(np.float32), rng.standard_normal((n, obs)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.01).astype(np.int8), np.zeros(n, np.int8))


def ring(obs, act, seed, fill):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=RING, seed=seed), (obs,), np.float32, (act,), np.float32, device=0)
    rb.push(*fill)
    return rb


def online(args, bench, shape, prefix, group_cls, agent_cls, config, obs, act):
    doc = {"bench": bench, "shape": shape + f"; train mode, one ring of {RING} rows per member ({FILLED} to begin with), host f32 rows, C calls on prepared arrays",
           "window_steps": args.window, "legs": args.legs, "leg_seconds": args.leg_seconds, "unit_push": "member-pushes/s (median of the legs)",
           "unit_iter": "member-iterations/s (median of the legs); one iteration = group sample, push, group opt of every member",
           "bar": "at P = 8 and P = 64: group_min >= loop_max", "push": {}, "iter": {}, "lone": {}}
    L = _lib.lib()
    sample, push, opt, sync = (getattr(L, f"{prefix}_{f}") for f in ("sample", "push", "opt", "sync"))
    vp = C.c_void_p
    fill = rows(obs, act, FILLED, 0)
    for P in [int(x) for x in args.sizes.split(",")]:
        ga, gb, gp = (group_cls.build([config(i, True) for i in range(P)]) for _ in range(3))
        a_rings, b_rings, pa_rings, pb_rings = ([ring(obs, act, 100 + i, fill) for i in range(P)] for _ in range(4))
        cols = rows(obs, act, P, 1)
        ptrs = [(vp * P)(*[c[i:i + 1].ctypes.data for i in range(P)]) for c in cols]   # per field: one row per member
        each = [tuple(vp(c[i:i + 1].ctypes.data) for c in cols) for i in range(P)]
        codes = (C.c_int32 * P)(*[_lib.BDR_DTYPE_F32] * P)
        outs = np.empty((P, act), np.float32)
        out_ptrs = (vp * P)(*[outs[i:i + 1].ctypes.data for i in range(P)])
        hs = {id(rs): (vp * P)(*[r.handle for r in rs]) for rs in (a_rings, b_rings, pa_rings)}
        ga.opt(a_rings); gb.opt(b_rings)

        def group_push(g, rs):
            _lib.check(push(g.handle, hs[id(rs)], 1, ptrs[0], ptrs[2], codes, ptrs[1], ptrs[3], ptrs[4], ptrs[5]))

        def loop_push(rs):
            for r, (o, a, x, rew, t, u) in zip(rs, each): _lib.check(L.bdr_replay_push(r.handle, 1, o, a, x, rew, t, u))

        def iter_group():
            _lib.check(sample(ga.handle, None, 1, ptrs[0], codes, out_ptrs))
            group_push(ga, a_rings)
            _lib.check(opt(ga.handle, hs[id(a_rings)]))

        def iter_loop():
            _lib.check(sample(gb.handle, None, 1, ptrs[0], codes, out_ptrs))
            loop_push(b_rings)
            _lib.check(opt(gb.handle, hs[id(b_rings)]))

        def loop_push_sync():
            for r in pb_rings: r.read_rows(0, 0)      # (synchronises the ring's stream)
        group_push(gp, pa_rings)
        for key, m in (("push", measure(lambda: group_push(gp, pa_rings), gp.sync, lambda: loop_push(pb_rings), loop_push_sync, P, args.window, args.legs, args.leg_seconds)),
                       ("iter", measure(iter_group, ga.sync, iter_loop, gb.sync, P, args.window, args.legs, args.leg_seconds))):
            if P > 1:
                m["bar_met"] = bool(m["group_min_max"][0] >= m["loop_min_max"][1])
            doc[key][str(P)] = m
            print(P, key, m, flush=True)
        if P == 1:   # the group of one against the agent alone
            a, rb = agent_cls.build(config(0, True)), ring(obs, act, 100, fill)
            o, ac, x, rew, t, u = each[0]

            def iter_lone():
                _lib.check(L.bdr_agent_sample_raw(a.handle, None, 1, o, _lib.BDR_DTYPE_F32, 0, 0, out_ptrs[0], None))
                _lib.check(L.bdr_replay_push(rb.handle, 1, o, ac, x, rew, t, u))
                _lib.check(L.bdr_agent_opt(a.handle, rb.handle))
            m = measure(iter_group, ga.sync, iter_lone, a.sync, 1, args.window, args.legs, args.leg_seconds)
            doc["lone"]["1"] = m
            print(1, "group of one against the lone agent", m, flush=True)
            a.close(); rb.close()
        for g in (ga, gb, gp): g.close()
        for r in a_rings + b_rings + pa_rings + pb_rings: r.close()
    return doc
