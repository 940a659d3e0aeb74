"""The rule of a group acting call on the host alone (border_amd/csrc/group_act_plan.hpp): which members a call selects, where every
selected member's rows and results stand in the staging areas, the 64 MiB cap, and the draws of the noise stream each member takes.
The header has no HIP in it: it is compiled here with the host compiler into a program of its own and checked against an independent
restatement written in this file.  The three bdr_iql_group_*_default fillers are called with a NULL group, and header, _lib.py and
ffi.rs are checked on the new symbols."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from border_amd import _lib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "group_act_plan.hpp"

using namespace bdr;

// plan P n O A list|all n_sel [members...] ; f64[P] ; train[P] ; counters[P]
int main(int argc, char** argv)
{
    if (argc < 8 || strcmp(argv[1], "plan")) return 2;
    int at = 2;
    const unsigned P = (unsigned)strtoul(argv[at++], nullptr, 10);
    const unsigned long long n = strtoull(argv[at++], nullptr, 10);
    const int O = atoi(argv[at++]), A = atoi(argv[at++]);
    const bool list = !strcmp(argv[at++], "list");
    const unsigned n_sel = (unsigned)strtoul(argv[at++], nullptr, 10);
    std::vector<uint32_t> members;
    for (unsigned b = 0; list && b < n_sel; ++b) members.push_back((uint32_t)strtoul(argv[at++], nullptr, 10));
    std::vector<int> f64(P), train(P);
    std::vector<uint64_t> counters(P);
    if (strcmp(argv[at++], ";")) return 2;
    for (unsigned p = 0; p < P; ++p) f64[p] = atoi(argv[at++]);
    if (strcmp(argv[at++], ";")) return 2;
    for (unsigned p = 0; p < P; ++p) train[p] = atoi(argv[at++]);
    if (strcmp(argv[at++], ";")) return 2;
    for (unsigned p = 0; p < P; ++p) counters[p] = strtoull(argv[at++], nullptr, 10);
    if (at != argc) return 2;
    const uint32_t* m = list ? members.data() : nullptr;
    const GaSelect s = ga_select(m, n_sel, P);
    printf("select %d %u\n", s.refusal, s.entry);
    const GaPlan pl = ga_plan(m, n_sel, P, n, O, A, f64.data());
    printf("refusal %d\n", pl.refusal);
    printf("cap %zu\n", GA_STAGE_MAX);
    if (pl.refusal == GA_OK || pl.refusal == GA_CAP) {
        printf("staged %zu\nres_floats %zu\n", pl.staged, pl.res_floats);
        for (size_t b = 0; b < pl.row_off.size(); ++b) printf("block %u %zu %zu\n", ga_member_at(m, (uint32_t)b), pl.row_off[b], pl.res_off[b]);
    }
    std::vector<uint64_t> start(n_sel ? n_sel : 1, 0);
    ga_apply_draws(pl, m, n_sel, n, A, train.data(), counters.data(), start.data());
    for (unsigned p = 0; p < P; ++p) printf("counter %u %llu\n", p, (unsigned long long)counters[p]);
    if (pl.refusal == GA_OK) for (unsigned b = 0; b < n_sel; ++b) printf("start %u %llu\n", ga_member_at(m, b), (unsigned long long)start[b]);
    for (unsigned p = 0; p < P; ++p) {
        bool selected = !list;
        for (uint32_t x : members) selected = selected || x == p;
        printf("draws %u %llu\n", p, (unsigned long long)ga_draws(selected, train[p] != 0, n, A));
    }
    return 0;
}
"""

OK, EMPTY, RANGE, ORDER, COUNT, ROWS, CAP = range(7)   # GaRefusal's order
STAGE_MAX = 64 << 20


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("group_act_plan")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "group_act_plan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def run(prog, P, n, O, A, members, f64, train, counters, n_sel=None):
    sel = ["all", P if n_sel is None else n_sel] if members is None else ["list", len(members)] + list(members)
    args = ["plan", P, n, O, A] + sel + [";"] + list(f64) + [";"] + list(train) + [";"] + list(counters)
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr, args)
    out = {"blocks": [], "counters": {}, "start": {}, "draws": {}}
    for line in r.stdout.splitlines():
        k, *v = line.split()
        v = [int(x) for x in v]
        if k == "block": out["blocks"].append(tuple(v))
        elif k in ("counter", "start", "draws"): out[k + "s" if k == "counter" else k][v[0]] = v[1]
        elif k == "select": out[k] = tuple(v)
        else: out[k] = v[0]
    return out


# ---- the restatement: written from the contract in include/border_amd.h, not from the header under test ------------------------------
def expect_select(members, n_sel, P):
    if n_sel < 1: return (EMPTY, 0)
    if members is not None:
        for b, m in enumerate(members):
            if m >= P: return (RANGE, b)
            if b and m <= members[b - 1]: return (ORDER, b)
    elif n_sel != P: return (COUNT, 0)
    return (OK, 0)


def expect_blocks(members, P, n, O, A, f64):
    sel = list(range(P)) if members is None else list(members)
    blocks, off = [], 0
    for b, p in enumerate(sel):
        blocks.append((p, off, b * n * A))
        nbytes = n * O * (8 if f64[p] else 4)
        off += -(-nbytes // 16) * 16
    return blocks, off, len(sel) * n * A


def test_selection_rules(prog):
    P, zeros = 5, [0] * 5
    cases = [([], EMPTY, 0), ([2, 1], ORDER, 1), ([2, 2], ORDER, 1), ([0, 5], RANGE, 1), ([7], RANGE, 0), ([0, 3], OK, 0), ([4], OK, 0),
             ([0, 1, 2, 3, 4], OK, 0), ([1, 3, 2], ORDER, 2), ([1, 9, 0], RANGE, 1)]
    for members, refusal, entry in cases:
        got = run(prog, P, 2, 17, 6, members, zeros, zeros, zeros)
        assert got["select"] == (refusal, entry) == expect_select(members, len(members), P), members
        assert got["refusal"] == refusal
    for n_sel, refusal in ((5, OK), (4, COUNT), (6, COUNT), (0, EMPTY)):      # without a list every member acts: n_sel must be P
        got = run(prog, P, 2, 17, 6, None, zeros, zeros, zeros, n_sel=n_sel)
        assert got["select"] == (refusal, 0) == expect_select(None, n_sel, P) and got["refusal"] == refusal, n_sel
    for n, refusal in ((0, ROWS), (1, OK), (65536, OK), (65537, ROWS)):
        assert run(prog, 2, n, 3, 1, None, [0, 0], [0, 0], [0, 0])["refusal"] == refusal, n


@pytest.mark.parametrize("members", [None, [0, 3], [1, 2, 4], [4]])
@pytest.mark.parametrize("n,O,A", [(1, 17, 6), (33, 45, 24), (32, 9, 4), (3, 21, 65), (3000, 17, 6)])
def test_staged_offsets_are_16_byte_aligned_blocks_in_selection_order(prog, members, n, O, A):
    P, f64 = 5, [0, 1, 1, 0, 1]
    got = run(prog, P, n, O, A, members, f64, [0] * P, [0] * P)
    blocks, staged, res = expect_blocks(members, P, n, O, A, f64)
    assert got["refusal"] == OK and got["blocks"] == blocks and got["staged"] == staged and got["res_floats"] == res
    assert all(off % 16 == 0 for _, off, _ in got["blocks"]) and staged % 16 == 0
    # blocks do not overlap: every member has a block of its own, also two members that name one host pointer (the plan never sees
    # pointers: one block per selected member, whatever it is filled from)
    ends = [off + n * O * (8 if f64[p] else 4) for p, off, _ in got["blocks"]]
    assert all(e <= nxt[1] for e, nxt in zip(ends, got["blocks"][1:])) and ends[-1] <= staged
    assert [r for _, _, r in got["blocks"]] == [b * n * A for b in range(len(got["blocks"]))]


def test_the_64_mib_cap_on_rows_and_on_results(prog):
    assert run(prog, 1, 1, 1, 1, None, [0], [0], [0])["cap"] == STAGE_MAX
    # rows: 3 x 65536 x 45 x 8 bytes = 70 778 880 > 64 MiB; as f32 rows the same call fits (35 389 440)
    assert run(prog, 3, 65536, 45, 24, None, [1, 1, 1], [0] * 3, [0] * 3)["refusal"] == CAP
    assert run(prog, 3, 65536, 45, 24, None, [0, 0, 0], [0] * 3, [0] * 3)["refusal"] == OK
    # exactly at the cap: 2 x 65536 x 64 x 8 bytes = 64 MiB of rows is accepted, one more member is not
    assert run(prog, 2, 65536, 64, 1, None, [1, 1], [0] * 2, [0] * 2)["staged"] == STAGE_MAX
    assert run(prog, 2, 65536, 64, 1, None, [1, 1], [0] * 2, [0] * 2)["refusal"] == OK
    assert run(prog, 3, 65536, 64, 1, [0, 1, 2], [1, 1, 0], [0] * 3, [0] * 3)["refusal"] == CAP
    # results: 2 x 65536 x 200 floats = 104 857 600 bytes > 64 MiB although the rows (2 x 65536 x 4 x 4) are small
    got = run(prog, 2, 65536, 4, 200, None, [0, 0], [0] * 2, [0] * 2)
    assert got["refusal"] == CAP and got["staged"] == 2 * 65536 * 16 and got["res_floats"] * 4 > STAGE_MAX
    assert run(prog, 2, 65536, 4, 128, None, [0, 0], [0] * 2, [0] * 2)["refusal"] == OK      # 2 x 65536 x 128 x 4 = 64 MiB exactly


def test_draws_per_member_with_mixed_modes_and_a_subset(prog):
    P, n, A = 5, 33, 6
    train, counters = [1, 0, 1, 1, 0], [100, 200, 300, 400, 500]
    got = run(prog, P, n, 17, A, [0, 1, 3], [0] * P, train, counters)
    assert got["refusal"] == OK
    assert got["draws"] == {0: n * A, 1: 0, 2: 0, 3: n * A, 4: 0}             # train: n * A; eval: 0; not selected: 0
    assert got["counters"] == {0: 100 + n * A, 1: 200, 2: 300, 3: 400 + n * A, 4: 500}
    assert got["start"] == {0: 100, 1: 200, 3: 400}                           # the call draws at the counter it found
    got = run(prog, P, 1, 17, A, None, [0] * P, train, counters)
    assert got["counters"] == {p: counters[p] + (A if train[p] else 0) for p in range(P)}


def test_a_refused_plan_leaves_every_counter_unchanged(prog):
    P, A = 3, 24
    train, counters = [1, 1, 1], [7, 8, 9]
    for kw in (dict(members=[2, 1], n=2), dict(members=[], n=2), dict(members=[0, 3], n=2), dict(members=None, n=0), dict(members=None, n=65537),
               dict(members=None, n=2, n_sel=2), dict(members=None, n=65536, f64=[1, 1, 1])):
        got = run(prog, P, kw["n"], 45, A, kw["members"], kw.get("f64", [0] * P), train, counters, n_sel=kw.get("n_sel"))
        assert got["refusal"] != OK and got["counters"] == dict(enumerate(counters)) and got["start"] == {}, kw


# ---- the IQL fillers with a NULL group --------------------------------------------------------------------------------------------------
def test_the_iql_default_fillers_produce_the_tables_without_a_group():
    L = _lib.lib()
    ops = _lib.BcGroupEvalOps()
    ops.n_members = 9
    L.bdr_iql_group_eval_ops_default(C.byref(ops), None)
    assert ops.n_members == 0 and bool(ops.sample_members) and not ops.group
    t = _lib.GroupTrainerOps()
    bufs = (C.c_void_p * 1)(None)
    L.bdr_iql_group_trainer_ops_default(C.byref(t), None, bufs)
    assert t.n_members == 0 and all(bool(getattr(t, f)) for f in ("set_train", "opt", "opt_with_record"))
    assert not bool(t.sample) and not bool(t.push)
    post = _lib.BcGroupTrainerPostC()
    L.bdr_iql_group_trainer_post_default(C.byref(post), None)
    assert bool(post.save_member) and bool(post.eval_ops.sample_members) and post.eval_ops.n_members == 0
    assert post.eval_interval == 0 and post.save_interval == 0
    # IQL's tables are not BC's: the hooks differ, so check_bc_group_eval and the NULL save_member fallback can tell them apart
    bc, bc_post = _lib.BcGroupEvalOps(), _lib.BcGroupTrainerPostC()
    L.bdr_bc_group_eval_ops_default(C.byref(bc), None)
    L.bdr_bc_group_trainer_post_default(C.byref(bc_post), None)
    addr = lambda f: C.cast(f, C.c_void_p).value
    assert addr(bc.sample_members) != addr(ops.sample_members) and addr(bc_post.save_member) != addr(post.save_member)


# ---- the symbols ------------------------------------------------------------------------------------------------------------------------
def test_header_lib_and_rust_shim_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    syms = ("bdr_iql_group_sample", "bdr_iql_group_sample_members", "bdr_iql_group_eval_ops_default", "bdr_iql_group_trainer_ops_default",
            "bdr_iql_group_trainer_post_default")
    from tests.test_rust_shim_layout import parse_c, parse_rs
    cf, rf = parse_c(header)[1], parse_rs(ffi)[1]
    for sym in syms:
        assert re.search(r"BDR_API \w+ %s\(" % sym, header), sym
        assert sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym), sym
        assert re.search(r"pub fn %s\(" % sym, ffi), sym
        assert cf[sym] == rf[sym], sym
        assert len(cf[sym][0]) == len(getattr(_lib.lib(), sym).argtypes), sym
        assert cf[sym][1] == ("()" if sym.endswith("_default") else "i32"), sym
    # the IQL pair has the BC pair's signature, the group type apart
    for a, b in (("bdr_iql_group_sample", "bdr_bc_group_sample"), ("bdr_iql_group_sample_members", "bdr_bc_group_sample_members")):
        assert cf[a][0][1:] == cf[b][0][1:] and cf[a][1] == cf[b][1], a
    group_rs = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
    iql_part = group_rs[group_rs.index("pub struct AmdIqlGroup"):]
    for method in ("pub fn sample(", "pub fn sample_members(", "pub fn evaluate(", "pub fn train_offline("):
        assert method in iql_part, method
    from border_amd.group import BcGroup, IqlGroup
    for method in ("sample", "evaluate", "train_offline"):
        assert callable(getattr(IqlGroup, method)) and callable(getattr(BcGroup, method)), method
