"""The compiled online loop of the continuous-action groups (csrc/trainer.hip bdr_trainer_train_cgroup_post) with counting stub tables -
no GPU involved: its refusals, the call order of an iteration, post == NULL, the observation dtypes it hands on, and the agreement of
include/border_amd.h, border_amd/_lib.py and the Rust shim's ffi.rs on bdr_cgroup_trainer_ops and the new symbols.  (The i64 loop shares
the loop body: tests/test_group_trainer_host.py and tests/test_group_eval_host.py keep passing unchanged.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from border_amd import _lib
from border_amd.trainer import NativeTrainer, TrainerConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "border_amd.h")
P, A = 3, 2
DTYPES = [np.float32, np.float64, np.float32]
ROWS = [16, 24, 24]   # bytes per member: 4 f32, 3 f64, 6 f32
NO_OBSERVER = C.cast(None, _lib.GROUP_OBSERVER_FN)


def first(ptrs, p, dt):
    return float(C.cast(ptrs[p], C.POINTER(C.c_double if dt == np.float64 else C.c_float))[0])


class Stub:
    """One log for the table's calls and the environments' calls.  Member p's action row is [100 p + k, -(100 p + k)] at the k-th sample
    call; its environment writes rows filled with its own step counter (offset 1000 p) and is done every 4 + p steps."""
    def __init__(self, obs_on_device=0):
        self.log, self.pushed, self.n_sample, self.t, self.keep = [], [], 0, [1000 * p for p in range(P)], []
        self.vts = (_lib.EnvVtable * P)(*[self._vt(p, obs_on_device) for p in range(P)])

    def ops(self):
        def set_train(_g, on):
            self.log.append(("train", on)); return 0

        def sample(_g, rows, dtypes, act_out):
            self.n_sample += 1
            self.log.append(("sample", tuple(first(rows, p, DTYPES[p]) for p in range(P)), tuple(dtypes[p] for p in range(P))))
            for p in range(P):
                row = C.cast(act_out[p], C.POINTER(C.c_float))
                row[0], row[1] = 100 * p + self.n_sample, -(100 * p + self.n_sample)
            return 0

        def push(_g, bufs, rows, next_rows, dtypes, act, reward, term, trunc):
            self.log.append(("push",))
            f = lambda ptrs, p, t: C.cast(ptrs[p], C.POINTER(t))
            self.pushed.append([(first(rows, p, DTYPES[p]), tuple(f(act, p, C.c_float)[j] for j in range(A)), first(next_rows, p, DTYPES[p]),
                                 f(reward, p, C.c_float)[0], f(term, p, C.c_int8)[0], f(trunc, p, C.c_int8)[0], dtypes[p]) for p in range(P)])
            assert [bufs[p] for p in range(P)] == [11, 22, 33]
            return 0

        def opt(_g, bufs):
            self.log.append(("opt",)); return 0

        def opt_rec(_g, bufs, out, cap, n):
            self.log.append(("opt_rec",))
            for p in range(P):
                out[p * cap], n[p] = 1.25 + p, 1
            return 0
        self._bufs = (C.c_void_p * P)(11, 22, 33)
        self.keep.append((_lib.G_SET_TRAIN_FN(set_train), _lib.CG_SAMPLE_FN(sample), _lib.CG_PUSH_FN(push), _lib.G_OPT_FN(opt), _lib.G_OPT_REC_FN(opt_rec)))
        return _lib.CGroupTrainerOps(None, self._bufs, P, 0, *self.keep[-1])

    def _vt(self, p, obs_on_device):
        def put(ptr):
            self.t[p] += 1
            row = np.full(ROWS[p] // np.dtype(DTYPES[p]).itemsize, self.t[p], DTYPES[p])
            C.memmove(ptr, row.ctypes.data, ROWS[p])

        def reset(_c, obs_out):
            self.log.append(("reset", p)); put(obs_out); return 0

        def step(_c, act, obs_out, reward, term, trunc, init_out):
            a = C.cast(act, C.POINTER(C.c_float))
            self.log.append(("step", p, a[0], a[1]))
            put(obs_out)
            done = (self.t[p] % 1000) % (4 + p) == 0
            reward[0], term[0], trunc[0] = 0.5 * self.t[p], 1 if done else 0, 0
            if done: put(init_out)
            return 0
        fns = (_lib.ENV_RESET_FN(reset), _lib.ENV_STEP_FN(step))
        self.keep.append(fns)
        return _lib.EnvVtable(None, fns[0], fns[1], obs_on_device, 0)


def codes():
    return (C.c_int32 * P)(*[_lib.BDR_DTYPE_F64 if d == np.float64 else _lib.BDR_DTYPE_F32 for d in DTYPES])


def run(cfg, stub, act_row_bytes=4 * A, rows=ROWS, post=None, ops=None, observer=True):
    c = NativeTrainer(TrainerConfig(**cfg))._config(0, act_row_bytes)
    st = (_lib.TrainerStatsC * P)()
    events = []
    obs = _lib.GROUP_OBSERVER_FN(lambda _c, m, e, o, ev, sc, n: events.append((m, e, o, NativeTrainer.EVENTS[ev], [sc[i] for i in range(n)])))
    ops = ops if ops is not None else stub.ops()
    rc = _lib.lib().bdr_trainer_train_cgroup_post(C.byref(c), (C.c_uint64 * P)(*rows), codes(), C.byref(ops), stub.vts,
                                                  C.byref(post) if post is not None else None, obs if observer else NO_OBSERVER, None, st)
    return rc, st, events


CFG = dict(max_opts=5, opt_interval=2, warmup_period=3, record_agent_info_interval=2)


def test_call_order_of_an_iteration_and_the_transitions():
    stub = Stub()
    rc, st, events = run(CFG, stub)
    assert rc == 0
    log = stub.log
    assert log[0] == ("train", 1) and log[1:1 + P] == [("reset", p) for p in range(P)]
    body, i, n_iter, n_opt = log[1 + P:], 0, 0, 0
    while i < len(body):   # sample -> steps in member order -> push -> at most one opt
        n_iter += 1
        assert body[i][0] == "sample" and body[i][2] == tuple(codes()); i += 1
        assert body[i:i + P] == [("step", p, 100.0 * p + n_iter, -(100.0 * p + n_iter)) for p in range(P)]; i += P
        assert body[i] == ("push",); i += 1
        if i < len(body) and body[i][0] in ("opt", "opt_rec"):
            n_opt += 1
            assert body[i][0] == ("opt_rec" if n_opt % 2 == 0 else "opt"); i += 1
    assert n_opt == 5 and n_iter == 12 and [st[m].env_steps for m in range(P)] == [12] * P   # opts at env_steps 4, 6, 8, 10, 12
    for m in range(P):
        mine = [row[m] for row in stub.pushed]
        for (o, a, x, r, t, _u, dt), nxt in zip(mine, mine[1:]):
            assert nxt[0] == (x + 1 if t else x)          # prev_obs = init_obs / obs
        assert [q[1] for q in mine] == [(100.0 * m + it, -(100.0 * m + it)) for it in range(1, n_iter + 1)]
        assert all(q[3] == 0.5 * q[2] and q[6] == codes()[m] for q in mine)
        assert st[m].n_episodes == sum(q[4] for q in mine) and st[m].opt_steps == 5 and st[m].n_records == 2
        ev = [e[1:] for e in events if e[0] == m]
        assert [e[2] for e in ev] == ["skip"] * 3 + ["opt", "skip", "opt_record", "skip", "opt", "skip", "opt_record", "skip", "opt"]
        assert all(e[3] == ([1.25 + m] if e[2] == "opt_record" else []) for e in ev)
    # the group's sample saw every member's prev_obs, in the member's own dtype
    assert [x[1] for x in log if x[0] == "sample"] == [tuple(row[m][0] for m in range(P)) for row in stub.pushed]


def test_post_null_is_the_plain_loop():
    a, b = Stub(), Stub()
    rc_a, st_a, ev_a = run(CFG, a)
    post = _lib.BcGroupTrainerPostC()   # all zero: nothing to evaluate, nothing to save
    rc_b, st_b, ev_b = run(CFG, b, post=post)
    assert rc_a == rc_b == 0 and a.log == b.log and a.pushed == b.pushed and ev_a == ev_b
    assert [(s.env_steps, s.opt_steps, s.n_records, s.n_episodes) for s in st_a] == [(s.env_steps, s.opt_steps, s.n_records, s.n_episodes) for s in st_b]
    rc, st, ev = run(CFG, Stub(), observer=False)
    assert rc == 0 and ev == [] and st[2].opt_steps == 5


@pytest.mark.parametrize("field", ["set_train", "sample", "push", "opt", "opt_with_record"])
def test_an_incomplete_table_is_refused(field):
    stub = Stub()
    ops = stub.ops()
    setattr(ops, field, C.cast(None, dict(_lib.CGroupTrainerOps._fields_)[field]))
    rc, _, _ = run(dict(max_opts=2), stub, ops=ops)
    assert rc == 1 and stub.log == [] and b"incomplete" in _lib.lib().bdr_last_error()


@pytest.mark.parametrize("what", ["act_row_bytes_0", "act_row_bytes_6", "obs_on_device", "max_opts_0", "opt_interval_0", "obs_row_bytes_0", "post_without_dirs"])
def test_argument_checks(what):
    stub = Stub(obs_on_device=1 if what == "obs_on_device" else 0)
    kw, cfg = {}, dict(max_opts=2)
    if what.startswith("act_row_bytes"): kw["act_row_bytes"] = int(what[-1])
    if what == "max_opts_0": cfg = dict(max_opts=0)
    if what == "opt_interval_0": cfg = dict(max_opts=1, opt_interval=0)
    if what == "obs_row_bytes_0": kw["rows"] = [16, 0, 24]
    if what == "post_without_dirs":
        kw["post"] = _lib.BcGroupTrainerPostC()
        kw["post"].save_interval = 1
    rc, _, _ = run(cfg, stub, **kw)
    assert rc == 1 and stub.log == []   # BDR_ERR_INVALID before anything runs


def test_default_tables_point_at_the_group_entries():
    for kind in ("awac", "candle_sac"):
        ops = _lib.CGroupTrainerOps()
        bufs = (C.c_void_p * 1)(None)
        getattr(_lib.lib(), f"bdr_{kind}_group_ctrainer_ops_default")(C.byref(ops), None, bufs)
        assert ops.n_members == 0 and all(bool(getattr(ops, f)) for f in ("set_train", "sample", "push", "opt", "opt_with_record"))


def test_null_arguments_of_the_push_are_invalid():
    for kind in ("awac", "candle_sac"):
        assert getattr(_lib.lib(), f"bdr_{kind}_group_push")(None, None, 1, None, None, None, None, None, None, None) == 1
        assert b"null" in _lib.lib().bdr_last_error()
        assert getattr(_lib.lib(), f"bdr_{kind}_group_push_max_rows")(None, None, None, None) == 1


NEW_SYMBOLS = ("bdr_awac_group_push", "bdr_awac_group_push_max_rows", "bdr_candle_sac_group_push", "bdr_candle_sac_group_push_max_rows",
               "bdr_awac_group_ctrainer_ops_default", "bdr_candle_sac_group_ctrainer_ops_default", "bdr_trainer_train_cgroup_post")


def test_header_lib_and_rust_shim_agree_on_the_new_symbols():
    from tests.test_group_trainer_host import _c_fields
    from tests.test_rust_shim_layout import parse_c, parse_rs
    header = open(HEADER).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    cf, rf = parse_c(header)[1], parse_rs(ffi)[1]
    for sym in NEW_SYMBOLS:
        assert re.search(r"BDR_API \w+ %s\(" % sym, header), sym
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"pub fn %s\(" % sym, ffi), sym
        assert cf[sym] == rf[sym], sym
        assert len(cf[sym][0]) == len(getattr(_lib.lib(), sym).argtypes), sym
        assert cf[sym][1] == ("()" if sym.endswith("_default") else "i32"), sym
    fields = _c_fields(header, "bdr_cgroup_trainer_ops")
    assert fields == [f for f, _ in _lib.CGroupTrainerOps._fields_]
    rust = re.search(r"pub struct bdr_cgroup_trainer_ops \{(.*?)\n\}", ffi, re.S).group(1)
    assert re.findall(r"pub (\w+):", rust) == fields
    group_rs = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
    for sym in ("bdr_awac_group_push", "bdr_candle_sac_group_push", "bdr_trainer_train_cgroup_post"):
        assert "ffi::" + sym in group_rs, sym
    assert "bdr_trainer_train_cgroup_post" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = [f for f, _ in _lib.CGroupTrainerOps._fields_]
    assert fields == ["group", "buffers", "n_members", "reserved", "set_train", "sample", "push", "opt", "opt_with_record"]
    prog = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {", '  printf("%zu", sizeof(bdr_cgroup_trainer_ops));']
    prog += [f'  printf(" %zu", offsetof(bdr_cgroup_trainer_ops, {f}));' for f in fields]
    prog += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(prog))
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)])
    size, *offs = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(_lib.CGroupTrainerOps) == 64
    assert offs == [getattr(_lib.CGroupTrainerOps, f).offset for f in fields] == [0, 8, 16, 20, 24, 32, 40, 48, 56]
