"""The lockstep evaluator of a group (csrc/trainer.hip bdr_evaluate_group) and Trainer::post_process in the group loop
(bdr_trainer_train_group_post) against border-core/src/evaluator/default_evaluator.rs:64-88 and trainer.rs:231-264 with counting stub
tables - no GPU involved - and the agreement of include/border_amd.h, border_amd/_lib.py and the Rust shim's ffi.rs on the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from border_amd import _lib
from border_amd.evaluator import Evaluator
from border_amd.trainer import NativeTrainer, TrainerConfig
from tests.test_group_trainer_host import ROWS, P, StubEnvs, StubGroup, _c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BDR_ERR_INVALID = 1


class ScriptEnv:
    """Member m's evaluation environment: episodes given as lists of (reward, is_terminated, is_truncated) (or a callable ix -> list);
    the observation is [m, ix, t, 0] f32.  Every call goes into the log shared by all members."""
    def __init__(self, m, episodes, log, fail_at=None):
        self.m, self.episodes, self.log, self.fail_at = m, episodes if callable(episodes) else (lambda ix: episodes[ix]), log, fail_at
        self.cur, self.t, self.ix, self.n_steps = None, 0, -1, 0

    def reset_with_index(self, ix):
        self.log.append(("reset", self.m, ix))
        self.cur, self.t, self.ix = self.episodes(ix), 0, ix
        return np.array([self.m, ix, 0, 0], np.float32)

    def step(self, act):
        self.n_steps += 1
        if self.fail_at == self.n_steps:
            raise RuntimeError("boom")
        r, term, trunc = self.cur[self.t]
        self.t += 1
        self.log.append(("step", self.m, self.ix, self.t, int(act[0])))
        return np.array([self.m, self.ix, self.t, 0], np.float32), r, term, trunc


def evaluators(episodes, n_episodes, log, refs=None, fail_at=None):
    refs = refs or [None] * len(episodes)
    return [Evaluator(ScriptEnv(m, episodes[m], log, fail_at and fail_at.get(m)), n_episodes[m], obs_dim=4, act_dim=1, act_dtype=np.int64, ref_scores=refs[m])
            for m in range(len(episodes))]


class Acting:
    """sample_members: logs the member list and the selected members' rows; member p's action is 100 * p + the number of calls so far"""
    def __init__(self, log, n=P, fail_at=None):
        self.log, self.n, self.k, self.fail_at = log, n, 0, fail_at

        def sample(_g, members, n_sel, obs, act_out):
            self.k += 1
            sel = [members[b] for b in range(n_sel)]
            rows = [tuple(int(x) for x in np.frombuffer((C.c_char * 16).from_address(obs[p]), np.float32)[:3]) for p in sel]
            self.log.append(("sample", tuple(sel), tuple(rows)))
            for p in sel: act_out[p] = 100 * p + self.k
            return 17 if self.fail_at == self.k else 0
        self.fn = _lib.G_SAMPLE_MEMBERS_FN(sample)

    def ops(self):
        return _lib.GroupEvalOps(None, self.n, 0, self.fn)


def evaluate_group(evs, acting):
    arr = (_lib.EvaluatorC * len(evs))(*[e.c_struct() if isinstance(e, Evaluator) else e for e in evs])
    out = (_lib.EvalResultC * len(evs))()
    ops = acting.ops()
    return _lib.lib().bdr_evaluate_group(arr, C.byref(ops), out), out


def episode(n, reward=1.0, trunc=False):
    return [(reward, 0, 0)] * (n - 1) + [(reward, 0 if trunc else 1, 1 if trunc else 0)]


def lockstep_model(n_episodes, lengths):
    """the rounds of the issue's rule, written down independently: per round the resets, the selection, the steps"""
    ix, t, is_open, out, k = [0] * len(lengths), [0] * len(lengths), [False] * len(lengths), [], 0
    while True:
        for p in range(len(lengths)):
            if not is_open[p] and ix[p] < n_episodes[p]:
                out.append(("reset", p, ix[p])); is_open[p], t[p] = True, 0
        sel = [p for p in range(len(lengths)) if is_open[p]]
        if not sel: return out
        k += 1
        out.append(("sample", tuple(sel), tuple((p, ix[p], t[p]) for p in sel)))
        for p in sel:
            t[p] += 1
            out.append(("step", p, ix[p], t[p], 100 * p + k))
        for p in sel:
            if t[p] == lengths[p]: is_open[p] = False; ix[p] += 1


def test_call_order_and_the_shrinking_selection():
    n_eps, lengths = [1, 3, 2], [2, 3, 4]
    log = []
    # member 0 terminates, member 1 truncates, member 2 ends its first episode by both flags and its second by truncation
    eps = [[episode(2)], [episode(3, trunc=True)] * 3, [[(1.0, 0, 0)] * 3 + [(1.0, 1, 1)], episode(4, trunc=True)]]
    rc, out = evaluate_group(evaluators(eps, n_eps, log), Acting(log))
    assert rc == 0
    assert log == lockstep_model(n_eps, lengths)
    # the first two rounds and the round after member 0 has left, spelled out
    assert log[:7] == [("reset", 0, 0), ("reset", 1, 0), ("reset", 2, 0), ("sample", (0, 1, 2), ((0, 0, 0), (1, 0, 0), (2, 0, 0))),
                       ("step", 0, 0, 1, 1), ("step", 1, 0, 1, 101), ("step", 2, 0, 1, 201)]
    assert log[7:11] == [("sample", (0, 1, 2), ((0, 0, 1), (1, 0, 1), (2, 0, 1))), ("step", 0, 0, 2, 2), ("step", 1, 0, 2, 102), ("step", 2, 0, 2, 202)]
    assert log[11:14] == [("sample", (1, 2), ((1, 0, 2), (2, 0, 2))), ("step", 1, 0, 3, 103), ("step", 2, 0, 3, 203)]
    assert log[14:16] == [("reset", 1, 1), ("sample", (1, 2), ((1, 1, 0), (2, 0, 3)))]
    sels = [x[1] for x in log if x[0] == "sample"]
    assert sels == [(0, 1, 2)] * 2 + [(1, 2)] * 6 + [(1,)]          # 2, 9 and 8 steps: member 2 leaves after round 8, member 1 after round 9
    # no call reaches a finished member; every member sees bdr_evaluate's own sequence
    assert [x for x in log if x[0] != "sample" and x[1] == 0] == [("reset", 0, 0), ("step", 0, 0, 1, 1), ("step", 0, 0, 2, 2)]
    for m in range(3):
        assert [x[2] for x in log if x[0] == "reset" and x[1] == m] == list(range(n_eps[m]))
        assert [x[2:4] for x in log if x[0] == "step" and x[1] == m] == [(ix, t) for ix in range(n_eps[m]) for t in range(1, lengths[m] + 1)]
        assert (out[m].n_steps, out[m].n_episodes) == (n_eps[m] * lengths[m], n_eps[m])
        assert out[m].score == np.float32(np.float32(n_eps[m] * lengths[m]) / np.float32(n_eps[m])) and out[m].has_normalized == 0


def test_each_score_is_one_f32_accumulator_in_call_order():
    rewards = [1e8, 1.0, -1e8, 0.5, 0.25, 0.25, 0.25, 0.25]   # f32: 1e8 + 1 = 1e8, so the 1 is lost: 1.5; float64: 2.5
    eps0 = [[(r, 0, 0) for r in rewards[:3]] + [(rewards[3], 1, 0)], [(r, 0, 0) for r in rewards[4:7]] + [(rewards[7], 0, 1)]]
    eps1 = [[(3.0, 1, 0)], [(4.5, 0, 1)], [(0.125, 1, 0)]]
    eps2 = [[(0.1, 0, 0), (0.2, 0, 0), (0.3, 0, 1)]]
    log = []
    rc, out = evaluate_group(evaluators([eps0, eps1, eps2], [2, 3, 1], log, refs=[None, (-1.5, 9.25), None]), Acting(log))
    assert rc == 0

    def f32_sum(rs):
        acc = np.float32(0)
        for r in rs: acc = np.float32(acc + np.float32(r))
        return acc
    want0 = np.float32(f32_sum(rewards) / np.float32(2))
    assert float(sum(rewards)) / 2 != float(want0)
    assert out[0].score == want0 == np.float32(0.75) and out[0].has_normalized == 0
    score1 = np.float32(f32_sum([3.0, 4.5, 0.125]) / np.float32(3))
    assert out[1].score == score1 and out[1].has_normalized == 1
    assert out[1].normalized == np.float32((score1 - np.float32(-1.5)) / (np.float32(9.25) - np.float32(-1.5)))
    assert out[2].score == np.float32(f32_sum([0.1, 0.2, 0.3]) / np.float32(1)) and out[2].has_normalized == 0
    assert [(o.n_steps, o.n_episodes) for o in out] == [(8, 2), (3, 3), (3, 1)]


def last_error():
    return _lib.lib().bdr_last_error().decode()


@pytest.mark.parametrize("field,value", [("step", None), ("reset_with_index", None), ("n_episodes", 0), ("obs_row_bytes", 0), ("act_row_bytes", 4),
                                         ("obs_dtype", _lib.BDR_DTYPE_F64), ("norm", 1), ("obs_on_device", 1)])
def test_evaluate_group_refusals_name_the_member(field, value):
    log = []
    evs = evaluators([[episode(2)]] * 3, [1, 1, 1], log)
    arr = (_lib.EvaluatorC * 3)(*[e.c_struct() for e in evs])
    if field == "step": arr[1].env.step = C.cast(None, _lib.EVAL_STEP_FN)
    elif field == "reset_with_index": arr[1].env.reset_with_index = C.cast(None, _lib.EVAL_RESET_FN)
    elif field == "obs_on_device": arr[1].env.obs_on_device = 1
    else: setattr(arr[1], field, value)
    rc, _ = evaluate_group(list(arr), Acting(log))
    assert rc == BDR_ERR_INVALID and "member 1" in last_error(), last_error()
    assert log == []


def test_a_failing_environment_or_acting_call_stops_the_evaluation():
    log = []
    evs = evaluators([[episode(3)]] * 3, [1, 1, 1], log, fail_at={1: 2})
    rc, _ = evaluate_group(evs, Acting(log))
    assert rc == 99 and isinstance(evs[1].error, RuntimeError)
    assert log[-2:] == [("sample", (0, 1, 2), ((0, 0, 1), (1, 0, 1), (2, 0, 1))), ("step", 0, 0, 2, 2)]   # member 2 was not stepped any more
    log = []
    rc, _ = evaluate_group(evaluators([[episode(3)]] * 3, [1, 1, 1], log), Acting(log, fail_at=2))
    assert rc == 17 and [x[0] for x in log].count("sample") == 2 and log[-1][0] == "sample"
    rc, _ = evaluate_group(evaluators([[episode(3)]] * 3, [1, 1, 1], []), type("A", (), {"ops": lambda self: _lib.GroupEvalOps(None, 3, 0, C.cast(None, _lib.G_SAMPLE_MEMBERS_FN))})())
    assert rc == BDR_ERR_INVALID


# ---- bdr_trainer_train_group_post --------------------------------------------------------------------------------------------------
class Saves:
    def __init__(self, fail_at=None):
        self.calls, self.fail_at = [], fail_at
        self.fn = _lib.G_SAVE_MEMBER_FN(lambda _g, m, d: (self.calls.append((m, d.decode())), 23 if self.fail_at == len(self.calls) else 0)[1])


def run_post(cfg, scores=None, eval_interval=0, save_interval=0, post=True, with_dirs=True, with_evaluators=True, dirs=None, refs=None, stub=None, envs=None,
             eval_fail_at=None, entry="post"):
    """the group loop over StubGroup / StubEnvs; member m's k-th evaluation is one episode of one step with reward scores[m][k]"""
    stub, envs = stub or StubGroup(), envs or StubEnvs()
    c = NativeTrainer(TrainerConfig(**cfg))._config(0, 8)
    st = (_lib.TrainerStatsC * P)()
    events = []
    obs = _lib.GROUP_OBSERVER_FN(lambda _c, m, e, o, ev, sc, n: events.append((m, e, o, NativeTrainer.EVENTS[ev], [sc[i] for i in range(n)] if ev != 3 else n)))
    ops = stub.ops()
    saves, elog = Saves(), []
    keep = []
    L = _lib.lib()
    if entry == "plain":
        rc = L.bdr_trainer_train_group(C.byref(c), (C.c_uint64 * P)(*ROWS), C.byref(ops), envs.vts, obs, None, st)
    elif not post:
        rc = L.bdr_trainer_train_group_post(C.byref(c), (C.c_uint64 * P)(*ROWS), C.byref(ops), envs.vts, None, obs, None, st)
    else:
        post_c = _lib.GroupTrainerPostC()
        L.bdr_group_trainer_post_default(C.byref(post_c), None)
        assert bool(post_c.save_member) and bool(post_c.eval_ops.sample_members) and post_c.eval_ops.n_members == 0
        post_c.eval_interval, post_c.save_interval, post_c.save_member = eval_interval, save_interval, saves.fn
        count = [-1] * P

        def episodes(m):
            def f(ix):
                count[m] += 1
                return [(scores[m][count[m]], 1, 0)]
            return f
        evs = evaluators([episodes(m) for m in range(P)], [1] * P, elog, refs=refs)
        acting = Acting(stub.log, fail_at=eval_fail_at)
        inner = acting.fn

        def sample(g, members, n, obs_, act):   # the evaluation's acting calls, marked in the group's own log between the set_train calls
            rc_ = inner(g, members, n, obs_, act)
            stub.log[-1] = ("eval_sample", stub.log[-1][1])
            return rc_
        keep.append(_lib.G_SAMPLE_MEMBERS_FN(sample))
        post_c.eval_ops = _lib.GroupEvalOps(None, P, 0, keep[0])
        if with_evaluators:
            arr = (_lib.EvaluatorC * P)(*[e.c_struct() for e in evs])
            post_c.evaluators = arr
        if with_dirs:
            d = (C.c_char_p * P)(*[x if x is None else x.encode() for x in (dirs or [f"/models/m{m}" for m in range(P)])])
            post_c.model_dirs = d
        rc = L.bdr_trainer_train_group_post(C.byref(c), (C.c_uint64 * P)(*ROWS), C.byref(ops), envs.vts, C.byref(post_c), obs, None, st)
    return rc, st, events, stub, envs, saves


SCORES = [[1.0, 3.0, 3.0], [5.0, 2.0, 1.0], [1.0, 2.0, 3.0]]   # equal at the end / falling / rising


def test_post_processing_over_twelve_opt_steps():
    cfg = dict(max_opts=12, opt_interval=1, warmup_period=0, record_agent_info_interval=3, record_compute_cost_interval=4)
    rc, st, events, stub, envs, saves = run_post(cfg, SCORES, eval_interval=4, save_interval=6, refs=[None, (1.0, 5.0), None])
    assert rc == 0 and st[0].opt_steps == 12
    # EVAL events: per member in member order, with the member's scalars ({score, normalized} for the member with reference scores)
    evals = [(m, o, sc) for m, _, o, name, sc in events if name == "eval"]
    assert evals == [(m, o, [SCORES[m][k]] + ([(SCORES[m][k] - 1.0) / 4.0] if m == 1 else [])) for k, o in enumerate((4, 8, 12)) for m in range(P)]
    # within an iteration: every member's OPT / OPT_RECORD event, then every member's EVAL, then every member's COST
    for o in (4, 8, 12):
        names = [(m, name) for m, _, oo, name, _ in events if oo == o]
        opt = "opt_record" if o % 3 == 0 else "opt"
        assert names == [(m, opt) for m in range(P)] + [(m, "eval") for m in range(P)] + [(m, "cost") for m in range(P)], o
    # set_train(0) / set_train(1) around each evaluation, whatever the scores; one acting call per evaluation round, over all members
    kinds = [x for x in stub.log if x[0] in ("train", "eval_sample")]
    assert kinds == [("train", 1)] + [("train", 0), ("eval_sample", (0, 1, 2)), ("train", 1)] * 3
    seq = [x[0] for x in stub.log if x[0] in ("opt", "opt_rec", "eval_sample")]
    assert [i for i, s in enumerate(seq) if s == "eval_sample"] == [4, 9, 14]   # after the 4th, 8th and 12th opt
    # each member's own best (a strict >; the first evaluation is always saved), numbered saves of every member at 6 and 12
    assert saves.calls == ([(m, f"/models/m{m}/best") for m in range(P)] + [(m, f"/models/m{m}/6") for m in range(P)]
                           + [(0, "/models/m0/best"), (2, "/models/m2/best")] + [(2, "/models/m2/best")] + [(m, f"/models/m{m}/12") for m in range(P)])
    # the evaluation's environment steps are not the Trainer's
    assert [x[0] for x in stub.log].count("sample") == 12 and [x[0] for x in stub.log].count("push") == 12
    assert all(st[m].env_steps == 12 for m in range(P))


def test_the_first_evaluation_is_always_saved_as_best():
    rc, _, events, _, _, saves = run_post(dict(max_opts=2), [[-3e38, -3.1e38]] * P, eval_interval=1)
    assert rc == 0
    assert saves.calls == [(m, f"/models/m{m}/best") for m in range(P)]   # -3e38 > f32::MIN; the second, lower one is not saved
    assert [sc for m, _, _, n, sc in events if n == "eval" and m == 1] == [[float(np.float32(-3e38))], [float(np.float32(-3.1e38))]]


def test_interval_zero_means_never():
    rc, st, events, stub, _, saves = run_post(dict(max_opts=6), [[]] * P)
    assert rc == 0 and st[0].opt_steps == 6 and saves.calls == [] and not [e for e in events if e[3] == "eval"]
    assert [x for x in stub.log if x[0] == "train"] == [("train", 1)]
    rc, _, events, _, _, saves = run_post(dict(max_opts=6), [[]] * P, save_interval=4, with_evaluators=False)   # saves alone
    assert rc == 0 and saves.calls == [(m, f"/models/m{m}/4") for m in range(P)] and not [e for e in events if e[3] == "eval"]
    rc, _, events, _, _, saves = run_post(dict(max_opts=6), [[2.0, 1.0, 5.0]] * P, eval_interval=2)              # evaluations alone
    assert rc == 0 and saves.calls == [(m, f"/models/m{m}/best") for m in range(P)] * 2
    assert [o for m, _, o, n, _ in events if n == "eval" and m == 0] == [2, 4, 6]


def test_only_iterations_with_an_opt_step_post_process():
    cfg = dict(max_opts=4, opt_interval=3, warmup_period=4)
    rc, st, events, stub, _, saves = run_post(cfg, [[1.0, 0.5]] * P, eval_interval=2, save_interval=1)
    assert rc == 0 and st[0].opt_steps == 4 and st[0].env_steps == 15
    # opt steps at env steps 6, 9, 12, 15; opt_steps stays 2 over env steps 10 and 11 (2 % 2 == 0 there too): one evaluation per opt step
    assert [(e, o) for m, e, o, n, _ in events if n == "eval" and m == 2] == [(9, 2), (15, 4)]
    assert [d for m, d in saves.calls if m == 1] == ["/models/m1/1", "/models/m1/best", "/models/m1/2", "/models/m1/3", "/models/m1/4"]
    assert len([1 for m, _, _, n, _ in events if n == "skip" and m == 0]) == 11


def test_post_null_reproduces_the_group_loop():
    cfg = dict(max_opts=9, opt_interval=2, warmup_period=3, record_agent_info_interval=4, record_compute_cost_interval=3)

    def run(entry):
        rc, st, events, stub, envs, _ = run_post(cfg, post=False, entry=entry)
        assert rc == 0
        return events, stub.log, stub.pushed, envs.order, [(s.env_steps, s.opt_steps, s.n_records, s.n_episodes) for s in st]
    a, b = run("post"), run("plain")
    assert a == b and len(a[0]) > 0 and a[4][0][1] == 9


def test_post_argument_checks_before_anything_runs():
    ok = dict(max_opts=2)
    cases = [dict(eval_interval=1, with_evaluators=False),                         # an eval interval without evaluators
             dict(save_interval=1, with_dirs=False), dict(eval_interval=1, with_dirs=False),   # something to save without directories
             dict(save_interval=1, dirs=["/a", None, "/c"]), dict(eval_interval=1, dirs=["/a", None, "/c"])]
    for kw in cases:
        rc, _, events, stub, envs, saves = run_post(ok, [[1.0, 1.0]] * P, **kw)
        assert rc == BDR_ERR_INVALID and stub.log == [] and envs.order == [] and events == [] and saves.calls == [], kw
        if "dirs" in kw:
            assert "member 1" in last_error(), last_error()


def test_a_failure_inside_post_processing_ends_the_loop_with_its_status():
    rc, _, _, stub, _, saves = run_post(dict(max_opts=50), [[1.0] * 9] * P, eval_interval=2, eval_fail_at=2)
    assert rc == 17                                                                # the second evaluation's acting call
    assert [x[0] for x in stub.log].count("opt") == 4 and [x for x in stub.log if x[0] == "train"][-1] == ("train", 0)
    assert saves.calls == [(m, f"/models/m{m}/best") for m in range(P)]

    class Boom(ScriptEnv):
        def step(self, act):
            raise RuntimeError("boom")
    ev = [Evaluator(Boom(m, [episode(1)], []), 1, obs_dim=4, act_dim=1, act_dtype=np.int64) for m in range(P)]
    log = []
    rc, _ = evaluate_group(ev, Acting(log))
    assert rc == 99 and isinstance(ev[0].error, RuntimeError) and ev[1].error is None
    from border_amd.group import raise_first
    with pytest.raises(RuntimeError, match="boom"):
        raise_first(ev, rc)


def test_header_lib_and_rust_shim_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    syms = ("bdr_agent_group_sample_members", "bdr_group_eval_ops_default", "bdr_evaluate_group", "bdr_group_trainer_post_default",
            "bdr_trainer_train_group_post")
    from tests.test_rust_shim_layout import parse_c, parse_rs
    cf, rf = parse_c(header)[1], parse_rs(ffi)[1]
    for sym in syms:
        assert re.search(r"BDR_API \w+ %s\(" % sym, header), sym
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"pub fn %s\(" % sym, ffi), sym
        assert cf[sym] == rf[sym], sym
        assert len(cf[sym][0]) == len(getattr(_lib.lib(), sym).argtypes), sym
        assert cf[sym][1] == ("()" if sym.endswith("_default") else "i32"), sym
    for name, cls in (("bdr_group_eval_ops", _lib.GroupEvalOps), ("bdr_group_trainer_post", _lib.GroupTrainerPostC)):
        fields = _c_fields(header, name)
        assert fields == [f for f, _ in cls._fields_], name
        rust = re.search(r"pub struct %s \{(.*?)\n\}" % name, ffi, re.S).group(1)
        assert re.findall(r"pub (\w+):", rust) == fields, name
    assert "have no group form" not in header
    group_rs = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
    for method in ("pub fn sample_members(", "pub fn evaluate(", "pub fn train_post("):
        assert method in group_rs, method
