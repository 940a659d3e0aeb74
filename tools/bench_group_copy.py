"""copy_members of a BcGroup, IqlGroup, AwacGroup and CandleSacGroup (ONE launch of k_group_copy whatever the pairs, csrc/group_copy.hpp)
against what the library offered before it: per pair and per (model, role) bdr_agent_get_params of the source into
bdr_agent_set_params of the destination - a quiesce, a device-to-host copy and the layout transform, then the transform back, a
host-to-device copy and a synchronise - in one process, at the pen shapes of the kinds' own benchmarks (tools/bench_*_group.py), for
P = 8 and P = 64 members and P / 4 pairs per call (members 0 .. P/4 - 1 onto members P/2 .. P/2 + P/4 - 1).  Both sides call the C ABI
on arrays prepared ahead.  The loop moves the arenas only; copy_members also carries the step counters, which the loop cannot.

Protocol (tools/bench_dqn_group.py): warm-up, then five legs of 0.3 s per side, the two sides alternating, a synchronise per leg; the
figure is the median of the legs, the spread their min / max.  The bar: at P = 8 and P = 64 the group's worst leg is not slower than
the loop's best leg.
Also: update rounds/s of each group at P = 8 over views of one ring of 100 000 rows, five legs (the kinds' own opt benchmark), beside
the figure of profiles/bench_<kind>_group.json from before copy_members existed: the round itself has not moved.
Writes one JSON document (default profiles/bench_group_copy.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import border_amd as B  # noqa: E402
import bench_awac_group, bench_bc_group, bench_candle_sac_group, bench_iql_group  # noqa: E402,E401
from bench_dqn_group import legs  # noqa: E402
from border_amd import _lib  # noqa: E402

OBS, ACT, ROWS = 45, 24, 100_000
ROLES = (0, 100, 200, 300)
KINDS = {
    # name: (group class, its benchmark's member config, the (model, role) ids of the parameter views, the shape in words)
    "bc": (B.BcGroup, bench_bc_group.config, [r for r in ROLES], "bc_pen: obs 45, act 24, Mlp[256,256] Tanh, AdamW"),
    "iql": (B.IqlGroup, bench_iql_group.config, [m + r for m in (0, 1, 2, 5) for r in ROLES] + [3, 4], "pen: value / critic / actor Mlp[256,256,256], 2 critics"),
    "awac": (B.AwacGroup, lambda i: bench_awac_group.config(i, True), [m + r for m in (0, 1, 2) for r in ROLES] + [3, 4], "pen: critic / actor Mlp[256,256,256], 2 critics"),
    "candle_sac": (B.CandleSacGroup, lambda i: bench_candle_sac_group.config(i, True), [m + r for m in (0, 1, 2, 5) for r in ROLES] + [3, 4],
                   "pen: twin critics [256,256], Mlp2 actor [256,256], Auto entropy coefficient"),
}


def rates(a_step, a_sync, b_step, b_sync, per_step, n_legs, leg_s):
    """a = copy_members, b = the get_params / set_params loop: warm-up, then alternating legs"""
    for _ in range(50): a_step()
    a_sync()
    for _ in range(3): b_step()
    b_sync()
    la, lb = [], []
    for _ in range(n_legs):
        la += legs(a_step, a_sync, per_step, 1, leg_s, 20)
        lb += legs(b_step, b_sync, per_step, 1, leg_s, 1)
    res = {"group": statistics.median(la), "group_min_max": [min(la), max(la)], "loop": statistics.median(lb), "loop_min_max": [min(lb), max(lb)]}
    res["ratio"] = res["group"] / res["loop"]
    res["ratio_worst_case"] = min(la) / max(lb)
    res["group_call_us"] = 1e6 * per_step / res["group"]
    res["loop_call_us"] = 1e6 * per_step / res["loop"]
    return {k: (round(v, 2) if isinstance(v, float) else [round(x, 1) for x in v]) for k, v in res.items()}


def copy_bench(kind, P, args):
    cls, config, ids, _ = KINDS[kind]
    L = _lib.lib()
    g = cls.build([config(i) for i in range(P)])
    hs = [m.handle for m in g.members]
    pairs = [(i, P // 2 + i) for i in range(P // 4)]
    src, dst = np.array([s for s, _ in pairs], np.uint32), np.array([d for _, d in pairs], np.uint32)
    sp, dp = src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)
    copy = getattr(L, f"{g._PREFIX}_copy_members")
    counts = {}
    for w in ids:
        n = C.c_uint64()
        _lib.check(L.bdr_agent_param_count_of(hs[0], w, C.byref(n)))
        counts[w] = n.value
    bufs = {w: np.empty(n, np.float32) for w, n in counts.items()}
    ptrs = {w: b.ctypes.data_as(C.c_void_p) for w, b in bufs.items()}

    def group_call():
        _lib.check(copy(g.handle, sp, dp, len(pairs), 0))

    def loop_call():
        for s, d in pairs:
            for w in ids:
                _lib.check(L.bdr_agent_get_params(hs[s], w, ptrs[w], counts[w]))
                _lib.check(L.bdr_agent_set_params(hs[d], w, ptrs[w], counts[w]))
    # the two sides move the same parameters
    group_call(); g.sync()
    want = [g.members[P // 2].get_params(role=r) for r in ("param", "exp_avg_sq")]
    g.members[P // 2].set_params(np.zeros_like(want[0]))
    loop_call()
    assert all(np.array_equal(x, g.members[P // 2].get_params(role=r)) for x, r in zip(want, ("param", "exp_avg_sq"))), "the loop and the copy differ"
    n0 = g.kernel_launches
    group_call()
    assert g.kernel_launches == n0 + 1
    m = rates(group_call, g.sync, loop_call, g.sync, len(pairs), args.legs, args.leg_seconds)
    m.update({"pairs": len(pairs), "views_per_member": len(ids), "floats_per_member": int(sum(counts.values()))})
    m["bar_met"] = bool(m["group_min_max"][0] >= m["loop_min_max"][1])
    g.close()
    return m


def opt_bench(kind, owner, args):
    cls, config, _, _ = KINDS[kind]
    P = 8
    g = cls.build([config(i) for i in range(P)])
    views = [owner.view(100 + i) for i in range(P)]
    g.opt(views)
    for _ in range(50): g.opt()
    g.sync()
    ls = legs(g.opt, g.sync, 1, args.legs, args.leg_seconds, 20)
    before = json.load(open(os.path.join(HERE, "..", "profiles", f"bench_{kind}_group.json")))["opt"]["8"]
    out = {"rounds_per_s": round(statistics.median(ls), 1), "rounds_per_s_min_max": [round(min(ls), 1), round(max(ls), 1)],
           "before_rounds_per_s": round(before["group"] / P, 1), "before_rounds_per_s_min_max": [round(x / P, 1) for x in before["group_min_max"]],
           "before_from": f"profiles/bench_{kind}_group.json (its own run)", "launches_per_round": g.launches_per_round}
    out["ratio_to_before"] = round(out["rounds_per_s"] / out["before_rounds_per_s"], 4)
    g.close()
    for v in views: v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--sizes", default="8,64")
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--no-opt", action="store_true", help="skip the update rounds/s of the groups at P = 8")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "bench_group_copy.json"))
    args = ap.parse_args()
    doc = {"bench": "group_copy", "legs": args.legs, "leg_seconds": args.leg_seconds,
           "unit": "member-copies/s (pairs per second, median of the legs); group = copy_members of P / 4 pairs, one launch; loop = per pair and per (model, role) "
                   "bdr_agent_get_params of the source into bdr_agent_set_params of the destination",
           "bar": "at P = 8 and P = 64: group_min >= loop_max", "copy": {}, "opt_P8": {}}
    kinds = [k for k in args.kinds.split(",") if k]
    for kind in kinds:
        doc["copy"][kind] = {"shape": KINDS[kind][3]}
        for P in [int(x) for x in args.sizes.split(",")]:
            doc["copy"][kind][str(P)] = copy_bench(kind, P, args)
            print(kind, P, doc["copy"][kind][str(P)], flush=True)
    if not args.no_opt:
        rng = np.random.default_rng(0)
        owner = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=ROWS, seed=1), (OBS,), np.float32, (ACT,), np.float32, device=0)
        for _ in range(ROWS // 10_000):
            n = 10_000
            owner.push(rng.standard_normal((n, OBS)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ACT)).astype(np.float32),
                       rng.standard_normal((n, OBS)).astype(np.float32), rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.01).astype(np.int8),
                       np.zeros(n, np.int8))
        for kind in kinds:
            doc["opt_P8"][kind] = opt_bench(kind, owner, args)
            print(kind, "opt", doc["opt_P8"][kind], flush=True)
        owner.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(args.out))


if __name__ == "__main__":
    main()
