"""The lockstep evaluator of a BC group (csrc/trainer.hip bdr_evaluate_bc_group) and Trainer::train_offline with post_process for a
group (bdr_trainer_train_offline_group_post) with counting stub tables through the real library - no GPU involved: the lockstep order
against an independent model of the rule, the scores against per-member bdr_evaluate, every member's event sequence against
bdr_trainer_train_offline_post driven with stubs that return the same records and scores, every refusal with nothing called, and the
agreement of include/border_amd.h, border_amd/_lib.py and the Rust shim on the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from border_amd import _lib
from border_amd.evaluator import Evaluator
from border_amd.trainer import NativeTrainer, TrainerConfig
from tests.test_group_eval_host import Saves, ScriptEnv, episode, last_error, lockstep_model
from tests.test_group_trainer_host import P, StubGroup, _c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BDR_ERR_INVALID = 1
ACT_DIMS = [3, 1, 6]                                    # per member: action rows of 12, 4 and 24 bytes
DTYPES = [np.float32, np.float64, np.float64]           # per member: the environment's rows
NORMS = [None, 0x5000, None]                            # per member: a normaliser handle (never dereferenced by the loop)


def evaluators(episodes, n_episodes, log, refs=None, fail_at=None, dtypes=DTYPES, act_dims=ACT_DIMS):
    refs = refs or [None] * len(episodes)
    return [Evaluator(ScriptEnv(m, episodes[m], log, fail_at and fail_at.get(m)), n_episodes[m], obs_dim=4, act_dim=act_dims[m], act_dtype=np.float32,
                      obs_dtype=dtypes[m], ref_scores=refs[m]) for m in range(len(episodes))]


def c_array(evs, norms=NORMS):
    arr = (_lib.EvaluatorC * len(evs))(*[e.c_struct() for e in evs])
    for m, h in enumerate(norms or []):
        if h is not None: arr[m].norm = h
    return arr


class Acting:
    """sample_members of a BC group: logs the member list and the selected members' rows as Acting of test_group_eval_host does, and in
    `seen` what else reaches the hook; member p's action row is [100 * p + the number of calls so far] * act_dim"""
    def __init__(self, log, n=P, fail_at=None, dtypes=DTYPES, act_dims=ACT_DIMS):
        self.log, self.n, self.k, self.fail_at, self.seen = log, n, 0, fail_at, []

        def sample(_g, members, n_sel, norms, rows, codes, act_out):
            self.k += 1
            sel = [members[b] for b in range(n_sel)]
            got = []
            for p in sel:
                dt = np.float64 if codes[p] == _lib.BDR_DTYPE_F64 else np.float32
                got.append(tuple(int(x) for x in np.frombuffer((C.c_char * (4 * np.dtype(dt).itemsize)).from_address(rows[p]), dt)[:3]))
                self.seen.append((p, codes[p], norms[p]))
                out = C.cast(act_out[p], C.POINTER(C.c_float))
                for j in range(act_dims[p]): out[j] = 100 * p + self.k
            self.log.append(("sample", tuple(sel), tuple(got)))
            return 17 if self.fail_at == self.k else 0
        self.fn = _lib.BG_SAMPLE_MEMBERS_FN(sample)

    def ops(self):
        return _lib.BcGroupEvalOps(None, self.n, 0, self.fn)


def evaluate_bc_group(arr, acting):
    out = (_lib.EvalResultC * len(arr))()
    ops = acting.ops()
    return _lib.lib().bdr_evaluate_bc_group(arr, C.byref(ops), out), out


# ---- the lockstep order ---------------------------------------------------------------------------------------------------------------
def test_lockstep_order_and_what_reaches_the_hook():
    n_eps, lengths = [1, 3, 2], [2, 3, 4]   # unequal episode counts and lengths; member 0 finishes first
    log = []
    eps = [[episode(2)], [episode(3, trunc=True)] * 3, [[(1.0, 0, 0)] * 3 + [(1.0, 1, 1)], episode(4, trunc=True)]]
    acting = Acting(log)
    rc, out = evaluate_bc_group(c_array(evaluators(eps, n_eps, log)), acting)
    assert rc == 0, last_error()
    assert log == lockstep_model(n_eps, lengths)
    sels = [x[1] for x in log if x[0] == "sample"]
    assert sels == [(0, 1, 2)] * 2 + [(1, 2)] * 6 + [(1,)]
    # every selected member's dtype and norm pointer, as its evaluator has them: float64 rows arrive as float64 (the row decoded above)
    assert set(acting.seen) == {(0, _lib.BDR_DTYPE_F32, None), (1, _lib.BDR_DTYPE_F64, 0x5000), (2, _lib.BDR_DTYPE_F64, None)}
    for m in range(3):
        assert [x[2] for x in log if x[0] == "reset" and x[1] == m] == list(range(n_eps[m]))
        assert [x[2:4] for x in log if x[0] == "step" and x[1] == m] == [(ix, t) for ix in range(n_eps[m]) for t in range(1, lengths[m] + 1)]
        assert (out[m].n_steps, out[m].n_episodes) == (n_eps[m] * lengths[m], n_eps[m])


def test_every_float_of_an_action_row_reaches_the_environment():
    seen = []

    class Env(ScriptEnv):
        def step(self, act):
            seen.append((self.m, act.tolist()))
            return super().step(act)
    log = []
    evs = [Evaluator(Env(m, [episode(2)], log), 1, obs_dim=4, act_dim=ACT_DIMS[m], act_dtype=np.float32, obs_dtype=DTYPES[m]) for m in range(P)]
    rc, _ = evaluate_bc_group(c_array(evs), Acting(log))
    assert rc == 0
    assert seen == [(m, [100.0 * m + k] * ACT_DIMS[m]) for k in (1, 2) for m in range(P)]


# ---- the scores -----------------------------------------------------------------------------------------------------------------------
def test_scores_equal_per_member_bdr_evaluate_as_f32_bits():
    rewards = [1e8, 1.0, -1e8, 0.5, 0.25, 0.25, 0.25, 0.25]   # f32: 1e8 + 1 = 1e8, so the 1 is lost
    eps = [[[(r, 0, 0) for r in rewards[:3]] + [(rewards[3], 1, 0)], [(r, 0, 0) for r in rewards[4:7]] + [(rewards[7], 0, 1)]],
           [[(3.0, 1, 0)], [(4.5, 0, 1)], [(0.125, 1, 0)]],
           [[(0.1, 0, 0), (0.2, 0, 0), (0.3, 0, 1)]]]
    n_eps, refs = [2, 3, 1], [None, (-1.5, 9.25), (0.0, 0.7)]
    rc, out = evaluate_bc_group(c_array(evaluators(eps, n_eps, [], refs=refs)), Acting([]))
    assert rc == 0
    raw = _lib.SAMPLE_RAW_FN(lambda *a: 0)
    plain = _lib.SAMPLE_FN(lambda *a: 0)
    for m in range(P):
        ev = c_array(evaluators(eps, n_eps, [], refs=refs))[m]
        ev.agent_sample_raw, ev.agent_sample = raw, plain
        one = _lib.EvalResultC()
        assert _lib.lib().bdr_evaluate(C.byref(ev), None, C.byref(one)) == 0
        for f in ("score", "normalized"):
            assert np.float32(getattr(out[m], f)).tobytes() == np.float32(getattr(one, f)).tobytes(), (m, f)
        assert (out[m].has_normalized, out[m].n_steps, out[m].n_episodes) == (one.has_normalized, one.n_steps, one.n_episodes)
    assert out[0].score == np.float32(0.75) and float(sum(rewards)) / 2 != 0.75


# ---- refusals of the evaluator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("step", None), ("reset_with_index", None), ("n_episodes", 0), ("obs_row_bytes", 0), ("act_row_bytes", 0),
                                         ("act_row_bytes", 6), ("obs_dtype", 7), ("obs_on_device", 1)])
def test_evaluate_bc_group_refusals_name_the_member(field, value):
    log = []
    arr = c_array(evaluators([[episode(2)]] * 3, [1, 1, 1], log))
    if field == "step": arr[1].env.step = C.cast(None, _lib.EVAL_STEP_FN)
    elif field == "reset_with_index": arr[1].env.reset_with_index = C.cast(None, _lib.EVAL_RESET_FN)
    elif field == "obs_on_device": arr[1].env.obs_on_device = 1
    else: setattr(arr[1], field, value)
    rc, _ = evaluate_bc_group(arr, Acting(log))
    assert rc == BDR_ERR_INVALID and "member 1" in last_error(), last_error()
    assert log == []


def test_incomplete_tables_and_the_default_table_are_refused_with_nothing_called():
    log = []
    arr = c_array(evaluators([[episode(2)]] * 3, [1, 1, 1], log))
    out = (_lib.EvalResultC * 3)()
    L = _lib.lib()
    for ops in (_lib.BcGroupEvalOps(None, 3, 0, C.cast(None, _lib.BG_SAMPLE_MEMBERS_FN)), _lib.BcGroupEvalOps(None, 0, 0, Acting(log).fn)):
        assert L.bdr_evaluate_bc_group(arr, C.byref(ops), out) == BDR_ERR_INVALID
    assert L.bdr_evaluate_bc_group(None, C.byref(Acting(log).ops()), out) == BDR_ERR_INVALID
    assert L.bdr_evaluate_bc_group(arr, None, out) == BDR_ERR_INVALID
    # the default table checks act_row_bytes against the member: without a group there is no member to check against
    ops = _lib.BcGroupEvalOps()
    L.bdr_bc_group_eval_ops_default(C.byref(ops), None)
    assert ops.n_members == 0 and bool(ops.sample_members)
    ops.n_members = 3
    assert L.bdr_evaluate_bc_group(arr, C.byref(ops), out) == BDR_ERR_INVALID and "member 0" in last_error()
    assert log == []


def test_a_failing_environment_or_acting_hook_returns_its_status_at_once():
    log = []
    evs = evaluators([[episode(3)]] * 3, [1, 1, 1], log, fail_at={1: 2})
    rc, _ = evaluate_bc_group(c_array(evs), Acting(log))
    assert rc == 99 and isinstance(evs[1].error, RuntimeError)
    assert log[-2:] == [("sample", (0, 1, 2), ((0, 0, 1), (1, 0, 1), (2, 0, 1))), ("step", 0, 0, 2, 2)]   # member 2 was not stepped any more
    log = []
    rc, _ = evaluate_bc_group(c_array(evaluators([[episode(3)]] * 3, [1, 1, 1], log)), Acting(log, fail_at=2))
    assert rc == 17 and [x[0] for x in log].count("sample") == 2 and log[-1][0] == "sample"


# ---- bdr_trainer_train_offline_group_post -----------------------------------------------------------------------------------------------
SCORES = [[1.0, 3.0, 3.0, 2.0], [5.0, 2.0, 1.0, 6.0], [1.0, 2.0, 3.0, 4.0]]   # equal after a rise / falling then a new best / rising
REFS = [None, (1.0, 5.0), None]


def scored(m, scores):
    """member m's k-th evaluation is one episode of one step with reward scores[m][k]"""
    count = [-1]

    def f(ix):
        count[0] += 1
        return [(scores[m][count[0]], 1, 0)]
    return f


def config(max_opts, record=0, cost=0):
    return NativeTrainer(TrainerConfig(max_opts=max_opts, record_agent_info_interval=record, record_compute_cost_interval=cost))._config(0, 0)


def event_log(events, with_member):
    def cb(_c, *a):
        m, (e, o, ev, sc, n) = (a[0], a[1:]) if with_member else (None, a)
        events.append((m, e, o, NativeTrainer.EVENTS[ev], [sc[i] for i in range(n)] if ev != 3 else n))   # (a COST record's scalars are times)
    return cb


def run_group(max_opts, record=0, cost=0, eval_interval=0, save_interval=0, post=True, with_dirs=True, with_evaluators=True, dirs=None, scores=SCORES,
              eval_fail_at=None, ops_edit=None, post_edit=None, evs_edit=None):
    stub = StubGroup()
    c = config(max_opts, record, cost)
    st = (_lib.TrainerStatsC * P)()
    events, elog = [], []
    obs = _lib.GROUP_OBSERVER_FN(event_log(events, True))
    ops = stub.ops()
    ops.sample, ops.push = C.cast(None, _lib.G_SAMPLE_FN), C.cast(None, _lib.G_PUSH_FN)   # not read by the offline loop
    if ops_edit: ops_edit(ops)
    saves, L = Saves(), _lib.lib()
    if not post:
        return L.bdr_trainer_train_offline_group_post(C.byref(c), C.byref(ops), None, obs, None, st), st, events, stub, saves, elog
    post_c = _lib.BcGroupTrainerPostC()
    L.bdr_bc_group_trainer_post_default(C.byref(post_c), None)
    assert bool(post_c.save_member) and bool(post_c.eval_ops.sample_members) and post_c.eval_ops.n_members == 0
    post_c.eval_interval, post_c.save_interval, post_c.save_member = eval_interval, save_interval, saves.fn
    acting = Acting(stub.log, fail_at=eval_fail_at)
    inner = acting.fn

    def sample(*a):   # the evaluation's acting calls, marked in the group's own log between the set_train calls
        rc_ = inner(*a)
        stub.log[-1] = ("eval_sample", stub.log[-1][1])
        return rc_
    keep = _lib.BG_SAMPLE_MEMBERS_FN(sample)
    post_c.eval_ops = _lib.BcGroupEvalOps(None, P, 0, keep)
    arr = c_array(evaluators([scored(m, scores) for m in range(P)], [1] * P, elog, refs=REFS))
    if evs_edit: evs_edit(arr)
    if with_evaluators: post_c.evaluators = arr
    d = (C.c_char_p * P)(*[x if x is None else x.encode() for x in (dirs or [f"/models/m{m}" for m in range(P)])])
    if with_dirs: post_c.model_dirs = d
    if post_edit: post_edit(post_c)
    rc = L.bdr_trainer_train_offline_group_post(C.byref(c), C.byref(ops), C.byref(post_c), obs, None, st)
    return rc, st, events, stub, saves, elog


def run_alone(m, max_opts, record, cost, eval_interval, save_interval, scores=SCORES):
    """bdr_trainer_train_offline_post of a lone agent whose stubs return member m's records and scores"""
    log, saved, events = [], [], []

    def opt_rec(_a, _b, out, cap, n):
        log.append(("opt_rec",))
        out[0], out[1], n[0] = 1.25 + m, -2.0, 2
        return 0
    fns = (_lib.SET_TRAIN_FN(lambda _a, on: (log.append(("train", on)), 0)[1]), _lib.SAMPLE_FN(lambda *a: 0), _lib.OPT_FN(lambda *a: (log.append(("opt",)), 0)[1]),
           _lib.OPT_REC_FN(opt_rec))
    ops = _lib.TrainerOps()
    ops.agent_set_train, ops.agent_sample, ops.agent_opt, ops.agent_opt_with_record = fns
    ev = evaluators([scored(i, scores) for i in range(P)], [1] * P, [], refs=REFS, dtypes=[np.float32] * P)[m]
    evc = ev.c_struct()
    evc.agent_sample = fns[1]
    save = _lib.SAVE_FN(lambda _a, d: (saved.append(d.decode()), 0)[1])
    post = _lib.TrainerPostC(eval_interval, save_interval, C.pointer(evc), f"/models/m{m}".encode(), save)
    c, st = config(max_opts, record, cost), _lib.TrainerStatsC()
    rc = _lib.lib().bdr_trainer_train_offline_post(C.byref(c), C.byref(ops), C.byref(post), _lib.OBSERVER_FN(event_log(events, False)), None, C.byref(st))
    assert rc == 0, last_error()
    return [e[1:] for e in events], saved, log, st


@pytest.mark.parametrize("max_opts,record,cost,eval_interval,save_interval", [(12, 3, 4, 4, 6),     # every interval divides max_opts
                                                                              (7, 4, 5, 2, 3),      # none does
                                                                              (5, 0, 0, 0, 0), (4, 1, 1, 1, 1)])
def test_every_member_sees_the_events_of_a_lone_offline_loop(max_opts, record, cost, eval_interval, save_interval):
    rc, st, events, stub, saves, _ = run_group(max_opts, record, cost, eval_interval, save_interval)
    assert rc == 0, last_error()
    for m in range(P):
        want_events, want_saved, want_log, want_st = run_alone(m, max_opts, record, cost, eval_interval, save_interval)
        assert [e[1:] for e in events if e[0] == m] == want_events, m
        assert [d for p, d in saves.calls if p == m] == want_saved, m
        assert [x for x in stub.log if x[0] != "eval_sample"] == want_log, m          # set_train, opt and opt_with_record: one decision for all
        assert (st[m].env_steps, st[m].opt_steps, st[m].n_records, st[m].n_episodes) == (want_st.env_steps, want_st.opt_steps, want_st.n_records, 0)
    n_eval = max_opts // eval_interval if eval_interval else 0
    # set_train: 1, then (0, 1) around every evaluation, whatever the scores; ONE acting call per evaluation round, over all members
    assert [x for x in stub.log if x[0] in ("train", "eval_sample")] == [("train", 1)] + [("train", 0), ("eval_sample", (0, 1, 2)), ("train", 1)] * n_eval
    assert st[0].opt_steps == max_opts == st[0].env_steps
    # within an iteration: every member's OPT / OPT_RECORD event, then every member's EVAL, then every member's COST, in member order
    for o in range(1, max_opts + 1):
        names = [(m, name) for m, _, oo, name, _ in events if oo == o]
        want = [(m, "opt_record" if record and o % record == 0 else "opt") for m in range(P)]
        if eval_interval and o % eval_interval == 0: want += [(m, "eval") for m in range(P)]
        if cost and o % cost == 0: want += [(m, "cost") for m in range(P)]
        assert names == want, o
    assert all(sc == [1.25 + m, -2.0] for m, _, _, name, sc in events if name == "opt_record")
    assert all(sc == 2 for _, _, _, name, sc in events if name == "cost")


def test_best_saves_follow_the_strict_greater_than():
    rc, _, events, _, saves, _ = run_group(8, eval_interval=2, save_interval=0)
    assert rc == 0
    # SCORES: member 0 1, 3, 3, 2 -> saved at 1 and the first 3; member 1 5, 2, 1, 6 -> 5 and 6; member 2 rises -> every time
    assert saves.calls == [(0, "/models/m0/best"), (1, "/models/m1/best"), (2, "/models/m2/best"), (0, "/models/m0/best"), (2, "/models/m2/best"),
                           (2, "/models/m2/best"), (1, "/models/m1/best"), (2, "/models/m2/best")]
    evals = [(m, o, sc) for m, _, o, name, sc in events if name == "eval"]
    assert evals == [(m, o, [SCORES[m][k]] + ([(SCORES[m][k] - 1.0) / 4.0] if m == 1 else [])) for k, o in enumerate((2, 4, 6, 8)) for m in range(P)]
    rc, _, _, _, saves, _ = run_group(2, eval_interval=1, scores=[[-3e38, -3.1e38]] * P)
    assert rc == 0 and saves.calls == [(m, f"/models/m{m}/best") for m in range(P)]   # -3e38 > f32::MIN; the second, lower one is not saved


def test_post_null_is_the_plain_offline_loop():
    rc, st, events, stub, saves, _ = run_group(6, record=4, cost=3, post=False)
    assert rc == 0 and saves.calls == [] and [x[0] for x in stub.log] == ["train", "opt", "opt", "opt", "opt_rec", "opt", "opt"]
    assert [(m, o, n) for m, _, o, n, _ in events] == [(m, o, n) for o in range(1, 7) for n in (["opt_record" if o == 4 else "opt"] + (["cost"] if o % 3 == 0 else []))
                                                       for m in range(P)]
    assert all(s.n_records == 1 and s.opt_steps == 6 for s in st)


def null_fn(field, kind):
    return lambda t: setattr(t, field, C.cast(None, kind))


@pytest.mark.parametrize("kw", [dict(max_opts=0), dict(ops_edit=null_fn("opt", _lib.G_OPT_FN)), dict(ops_edit=null_fn("opt_with_record", _lib.G_OPT_REC_FN)),
                                dict(ops_edit=null_fn("set_train", _lib.G_SET_TRAIN_FN)), dict(ops_edit=lambda o: setattr(o, "n_members", 0)),
                                dict(ops_edit=lambda o: setattr(o, "buffers", None)),
                                dict(eval_interval=1, with_evaluators=False), dict(save_interval=1, with_dirs=False), dict(eval_interval=1, with_dirs=False),
                                dict(save_interval=1, dirs=["/a", None, "/c"], names=1), dict(eval_interval=1, dirs=["/a", None, "/c"], names=1),
                                dict(eval_interval=1, post_edit=lambda p: setattr(p.eval_ops, "n_members", 2)),
                                dict(eval_interval=1, post_edit=lambda p: setattr(p.eval_ops, "sample_members", C.cast(None, _lib.BG_SAMPLE_MEMBERS_FN))),
                                dict(eval_interval=1, evs_edit=lambda a: setattr(a[1], "act_row_bytes", 6), names=1),
                                dict(eval_interval=1, evs_edit=lambda a: setattr(a[1].env, "obs_on_device", 1), names=1)])
def test_refusals_before_anything_runs(kw):
    kw = dict(kw)
    names = kw.pop("names", None)
    rc, _, events, stub, saves, elog = run_group(kw.pop("max_opts", 2), **kw)
    assert rc == BDR_ERR_INVALID and stub.log == [] and events == [] and saves.calls == [] and elog == [], (kw, last_error())
    if names is not None:
        assert f"member {names}" in last_error(), last_error()
    assert _lib.lib().bdr_trainer_train_offline_group_post(None, None, None, C.cast(None, _lib.GROUP_OBSERVER_FN), None, None) == BDR_ERR_INVALID


def test_a_failure_inside_the_loop_ends_it_with_its_status():
    rc, _, _, stub, saves, _ = run_group(50, eval_interval=2, eval_fail_at=2, scores=[[1.0] * 9] * P)
    assert rc == 17                                                                # the second evaluation's acting hook
    assert [x[0] for x in stub.log].count("opt") == 4 and [x for x in stub.log if x[0] == "train"][-1] == ("train", 0)
    assert saves.calls == [(m, f"/models/m{m}/best") for m in range(P)]
    stub = StubGroup(fail_at={("opt", 3): 23})
    ops = stub.ops()
    c = config(9)
    assert _lib.lib().bdr_trainer_train_offline_group_post(C.byref(c), C.byref(ops), None, C.cast(None, _lib.GROUP_OBSERVER_FN), None, None) == 23
    assert [x[0] for x in stub.log] == ["train", "opt", "opt", "opt"]


def test_the_default_tables_point_at_the_bc_group_entries():
    ops = _lib.GroupTrainerOps()
    bufs = (C.c_void_p * 1)(None)
    _lib.lib().bdr_bc_group_trainer_ops_default(C.byref(ops), None, bufs)
    assert ops.n_members == 0 and all(bool(getattr(ops, f)) for f in ("set_train", "opt", "opt_with_record"))
    assert not bool(ops.sample) and not bool(ops.push)


# ---- the symbols ------------------------------------------------------------------------------------------------------------------------
def test_header_lib_and_rust_shim_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    syms = ("bdr_bc_group_sample", "bdr_bc_group_sample_members", "bdr_bc_group_eval_ops_default", "bdr_evaluate_bc_group",
            "bdr_bc_group_trainer_ops_default", "bdr_bc_group_trainer_post_default", "bdr_trainer_train_offline_group_post")
    from tests.test_rust_shim_layout import parse_c, parse_rs
    cf, rf = parse_c(header)[1], parse_rs(ffi)[1]
    for sym in syms:
        assert re.search(r"BDR_API \w+ %s\(" % sym, header), sym
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"pub fn %s\(" % sym, ffi), sym
        assert cf[sym] == rf[sym], sym
        assert len(cf[sym][0]) == len(getattr(_lib.lib(), sym).argtypes), sym
        assert cf[sym][1] == ("()" if sym.endswith("_default") else "i32"), sym
    for name, cls in (("bdr_bc_group_eval_ops", _lib.BcGroupEvalOps), ("bdr_bc_group_trainer_post", _lib.BcGroupTrainerPostC)):
        fields = _c_fields(header, name)
        assert fields == [f for f, _ in cls._fields_], name
        rust = re.search(r"pub struct %s \{(.*?)\n\}" % name, ffi, re.S).group(1)
        assert re.findall(r"pub (\w+):", rust) == fields, name
    group_rs = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
    bc_part = group_rs[group_rs.index("pub struct AmdBcGroup"):]
    for method in ("pub fn sample(", "pub fn sample_members(", "pub fn evaluate(", "pub fn train_offline("):
        assert method in bc_part, method
    from border_amd.group import BcGroup
    for method in ("sample", "evaluate", "train_offline"):
        assert callable(getattr(BcGroup, method)), method
