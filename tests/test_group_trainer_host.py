"""The compiled group loop (csrc/trainer.hip bdr_trainer_train_group) against the rules of border-core/src/trainer.rs:197-228, 267-327
with counting stub tables - no GPU involved - and the agreement of include/border_amd.h, border_amd/_lib.py and the Rust shim's
ffi.rs on the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from border_amd import _lib
from border_amd.trainer import NativeTrainer, TrainerConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 3
ROWS = [16, 12, 24]   # bytes per member


class StubGroup:
    """Counts every call; member p's action is 100 * p + the number of sample calls so far."""
    def __init__(self, fail_at=None):
        self.log, self.pushed, self.n_sample, self.fail_at = [], [], 0, fail_at or {}

    def _status(self, what):
        n = sum(1 for x in self.log if x[0] == what)
        return self.fail_at.get((what, n), 0)

    def ops(self):
        def first(ptrs, p): return float(C.cast(ptrs[p], C.POINTER(C.c_float))[0])

        def set_train(_g, on):
            self.log.append(("train", on)); return self._status("train")

        def sample(_g, obs, act_out):
            self.n_sample += 1
            self.log.append(("sample", tuple(first(obs, p) for p in range(P))))
            for p in range(P): act_out[p] = 100 * p + self.n_sample
            return self._status("sample")

        def push(_g, bufs, obs, act, nobs, rew, term, trunc):
            self.log.append(("push",))
            self.pushed.append([(first(obs, p), int(act[p]), first(nobs, p), float(rew[p]), int(term[p]), int(trunc[p])) for p in range(P)])
            assert [bufs[p] for p in range(P)] == [11, 22, 33]
            return self._status("push")

        def opt(_g, bufs):
            self.log.append(("opt",)); return self._status("opt")

        def opt_rec(_g, bufs, out, cap, n):
            self.log.append(("opt_rec",))
            assert cap == 128
            for p in range(P):
                out[p * cap], out[p * cap + 1] = 1.25 + p, -2.0
                n[p] = 2
            return self._status("opt_rec")

        self._bufs = (C.c_void_p * P)(11, 22, 33)
        self._keep = (_lib.G_SET_TRAIN_FN(set_train), _lib.G_SAMPLE_FN(sample), _lib.G_PUSH_FN(push), _lib.G_OPT_FN(opt), _lib.G_OPT_REC_FN(opt_rec))
        return _lib.GroupTrainerOps(None, self._bufs, P, 0, *self._keep)


class StubEnvs:
    """member p: obs = [t, ...] f32 of its own step counter (offset 1000 * p), done every 4 + p steps; logs the order of the calls"""
    def __init__(self, fail_step=None, **flags):
        self.t, self.order, self.fail_step, self.keep = [1000 * p for p in range(P)], [], fail_step, []
        self.vts = (_lib.EnvVtable * P)(*[self._vt(p, **flags) for p in range(P)])

    def _vt(self, p, obs_on_device=0):
        def put(ptr):
            self.t[p] += 1
            C.memmove(ptr, np.full(ROWS[p] // 4, self.t[p], np.float32).ctypes.data, ROWS[p])

        def reset(_c, obs_out):
            self.order.append(("reset", p)); put(obs_out); return 0

        def step(_c, act, obs_out, reward, term, trunc, init_out):
            self.order.append(("step", p, C.c_int64.from_address(act).value))
            if self.fail_step == (p, sum(1 for o in self.order if o[0] == "step" and o[1] == p)):
                return 42
            put(obs_out)
            done = (self.t[p] % 1000) % (4 + p) == 0
            reward[0], term[0], trunc[0] = 0.5 * self.t[p], 1 if done else 0, 0
            if done: put(init_out)
            return 0
        fns = (_lib.ENV_RESET_FN(reset), _lib.ENV_STEP_FN(step))
        self.keep.append(fns)
        return _lib.EnvVtable(None, fns[0], fns[1], obs_on_device, 0)


def run(cfg, stub, envs, with_observer=True, rows=ROWS):
    c = NativeTrainer(TrainerConfig(**cfg))._config(0, 8)
    st = (_lib.TrainerStatsC * P)()
    events = []
    obs = _lib.GROUP_OBSERVER_FN(lambda _c, m, e, o, ev, sc, n: events.append((m, e, o, NativeTrainer.EVENTS[ev], [sc[i] for i in range(n)])))
    ops = stub.ops()
    rc = _lib.lib().bdr_trainer_train_group(C.byref(c), (C.c_uint64 * P)(*rows), C.byref(ops), envs.vts,
                                            obs if with_observer else C.cast(None, _lib.GROUP_OBSERVER_FN), None, st)
    return rc, st, events


@pytest.mark.parametrize("cfg", [dict(max_opts=7, opt_interval=1, warmup_period=0, record_agent_info_interval=3),
                                 dict(max_opts=5, opt_interval=4, warmup_period=10, record_agent_info_interval=2),
                                 dict(max_opts=3, opt_interval=3, warmup_period=7, record_agent_info_interval=0)])
def test_group_loop_rules(cfg):
    stub, envs = StubGroup(), StubEnvs()
    rc, st, events = run(cfg, stub, envs)
    assert rc == 0
    kinds = [x[0] for x in stub.log]
    # one set_train, then per iteration: sample, push, and at most one opt / opt_rec
    assert stub.log[0] == ("train", 1) and kinds.count("train") == 1
    n_iter = kinds.count("sample")
    assert kinds.count("push") == n_iter
    body = kinds[1:]
    i = 0
    for it in range(1, n_iter + 1):
        assert body[i:i + 2] == ["sample", "push"]; i += 2
        if i < len(body) and body[i] in ("opt", "opt_rec"): i += 1
    assert i == len(body)
    # the environments: reset once each in member order, then every step in member order with the member's own action
    assert envs.order[:P] == [("reset", p) for p in range(P)]
    steps = envs.order[P:]
    assert steps == [("step", p, 100 * p + it) for it in range(1, n_iter + 1) for p in range(P)]
    # train_step's rule (trainer.rs:197-228), one decision for all members
    first = max(cfg["warmup_period"], 1)
    first += (-first) % cfg["opt_interval"]
    opt_at = [first + k * cfg["opt_interval"] for k in range(cfg["max_opts"])]
    k = cfg["record_agent_info_interval"]
    rec_at = [o for o in range(1, cfg["max_opts"] + 1) if o % k == 0] if k else []
    assert n_iter == opt_at[-1]
    assert kinds.count("opt") + kinds.count("opt_rec") == cfg["max_opts"] and kinds.count("opt_rec") == len(rec_at)
    for m in range(P):
        mine = [e[1:] for e in events if e[0] == m]
        assert [e[0] for e in mine] == list(range(1, n_iter + 1))                        # one event per iteration and member
        assert [e[0] for e in mine if e[2] in ("opt", "opt_record")] == opt_at
        assert [e[1] for e in mine if e[2] == "opt_record"] == rec_at
        assert all(e[3] == ([1.25 + m, -2.0] if e[2] == "opt_record" else []) for e in mine)   # the member's own Record
        assert st[m].env_steps == n_iter and st[m].opt_steps == cfg["max_opts"] and st[m].n_records == len(rec_at)
    assert [e[0] for e in events[:P]] == list(range(P))                                  # member order within an iteration
    # transitions (step_proc.rs:103-137), per member: the chain continues from next_obs, restarts from init_obs after a done step
    for m in range(P):
        mine = [row[m] for row in stub.pushed]
        for (o, a, x, r, t, _), nxt in zip(mine, mine[1:]):
            assert nxt[0] == (x + 1 if t else x)
        assert [q[1] for q in mine] == [100 * m + it for it in range(1, n_iter + 1)]
        assert st[m].n_episodes == sum(q[4] for q in mine)
        assert all(q[3] == 0.5 * q[2] for q in mine)
    # the group's sample saw every member's prev_obs
    assert [x[1] for x in stub.log if x[0] == "sample"] == [tuple(row[m][0] for m in range(P)) for row in stub.pushed]
    if n_iter >= 8:
        assert len({st[m].n_episodes for m in range(P)}) > 1   # episodes of 4, 5 and 6 steps


def test_cost_records_and_no_observer():
    cfg = dict(max_opts=6, opt_interval=1, warmup_period=0, record_agent_info_interval=0, record_compute_cost_interval=3)
    rc, st, events = run(cfg, StubGroup(), StubEnvs())
    assert rc == 0
    cost = [e for e in events if e[3] == "cost"]
    assert [(e[0], e[2]) for e in cost] == [(m, o) for o in (3, 6) for m in range(P)] and all(len(e[4]) == 2 for e in cost)
    rc, st, events = run(cfg, StubGroup(), StubEnvs(), with_observer=False)
    assert rc == 0 and events == [] and st[2].opt_steps == 6


@pytest.mark.parametrize("what,n,calls", [("sample", 3, dict(sample=4, push=3, opt=2, opt_rec=1)), ("push", 2, dict(sample=3, push=3, opt=2, opt_rec=0)),
                                          ("opt", 1, dict(sample=2, push=2, opt=2)), ("opt_rec", 0, dict(sample=3, push=3, opt=2, opt_rec=1)),
                                          ("train", 0, dict(train=1, sample=0))])
def test_a_failing_callback_ends_the_loop_with_its_status(what, n, calls):
    stub = StubGroup(fail_at={(what, n + 1): 17})
    rc, st, _ = run(dict(max_opts=50, opt_interval=1, warmup_period=0, record_agent_info_interval=3), stub, StubEnvs())
    assert rc == 17
    kinds = [x[0] for x in stub.log]
    for k, v in calls.items():
        assert kinds.count(k) == v, (k, kinds)


def test_a_failing_environment_ends_the_loop_with_its_status():
    stub, envs = StubGroup(), StubEnvs(fail_step=(1, 4))
    rc, st, _ = run(dict(max_opts=50), stub, envs)
    assert rc == 42
    kinds = [x[0] for x in stub.log]
    assert kinds.count("push") == 3 and kinds.count("opt") == 3 and kinds.count("sample") == 4
    assert envs.order[-2:] == [("step", 0, 4), ("step", 1, 104)]   # member 2 was not stepped any more


def test_argument_checks():
    from border_amd import BdrError
    ok = dict(max_opts=2)
    for cfg, stub, envs, rows in ((dict(max_opts=0), StubGroup(), StubEnvs(), ROWS), (dict(max_opts=1, opt_interval=0), StubGroup(), StubEnvs(), ROWS),
                                  (ok, StubGroup(), StubEnvs(obs_on_device=1), ROWS), (ok, StubGroup(), StubEnvs(), [16, 0, 24])):
        rc, _, _ = run(cfg, stub, envs, rows=rows)
        assert rc != 0 and stub.log == [] and envs.order == []
        with pytest.raises(BdrError):
            _lib.check(rc)
    stub = StubGroup()
    ops = stub.ops()
    ops.push = C.cast(None, _lib.G_PUSH_FN)
    c = NativeTrainer(TrainerConfig(**ok))._config(0, 8)
    assert _lib.lib().bdr_trainer_train_group(C.byref(c), (C.c_uint64 * P)(*ROWS), C.byref(ops), StubEnvs().vts, C.cast(None, _lib.GROUP_OBSERVER_FN), None, None) != 0
    c = NativeTrainer(TrainerConfig(**ok))._config(0, 4)   # act_row_bytes
    ops = stub.ops()
    assert _lib.lib().bdr_trainer_train_group(C.byref(c), (C.c_uint64 * P)(*ROWS), C.byref(ops), StubEnvs().vts, C.cast(None, _lib.GROUP_OBSERVER_FN), None, None) != 0
    assert stub.log == []


def test_default_table_points_at_the_group_entries():
    ops = _lib.GroupTrainerOps()
    bufs = (C.c_void_p * 1)(None)
    _lib.lib().bdr_group_trainer_ops_default(C.byref(ops), None, bufs)
    assert ops.n_members == 0 and all(bool(getattr(ops, f)) for f in ("set_train", "sample", "push", "opt", "opt_with_record"))


def _c_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl: continue
        m = re.match(r"int32_t \(\*(\w+)\)", decl)
        out.append(m.group(1) if m else re.split(r"[ *]", decl)[-1])
    return out


def test_header_lib_and_rust_shim_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    for sym in ("bdr_agent_group_push", "bdr_group_trainer_ops_default", "bdr_trainer_train_group"):
        assert re.search(r"BDR_API \w+ %s\(" % sym, header), sym
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"pub fn %s\(" % sym, ffi), sym
    fields = _c_fields(header, "bdr_group_trainer_ops")
    assert fields == [f for f, _ in _lib.GroupTrainerOps._fields_]
    rust = re.search(r"pub struct bdr_group_trainer_ops \{(.*?)\n\}", ffi, re.S).group(1)
    assert re.findall(r"pub (\w+):", rust) == fields
    # signatures: the C declaration and the Rust declaration spelled alike, the ctypes argtypes as many
    from tests.test_rust_shim_layout import parse_c, parse_rs
    cf, rf = parse_c(header)[1], parse_rs(ffi)[1]
    for sym in ("bdr_agent_group_push", "bdr_trainer_train_group", "bdr_group_trainer_ops_default"):
        assert cf[sym] == rf[sym], sym
        assert len(cf[sym][0]) == len(getattr(_lib.lib(), sym).argtypes), sym
    assert cf["bdr_agent_group_push"][1] == cf["bdr_trainer_train_group"][1] == "i32" and cf["bdr_group_trainer_ops_default"][1] == "()"
