"""Prioritized replay under an agent group, the part that needs no GPU.

1. bdr_agent_group_set_prioritized is on every surface (header, library, _lib.ABI_SYMBOLS, ffi.rs, AmdDqnGroup, DqnGroup).
2. The tree rules the grouped kernels share with the single-ring ones (border_amd/csrc/per_tree.hpp: the descent with its staged top
   and three-level fetch, the ancestor-at-depth formula, the duplicate scan, the in-batch-order fold) run on the CPU:
   tools/group_per_sim.cpp - a stand-alone program with its own main, built with -fsanitize=address,undefined and run directly - drives
   them over bounds-checked arrays on the grouped kernels' schedules.  Expectation: oracle.oracle.SumTree, the sum_tree.rs restatement
   tests/test_gpu_per.py compares the device against.

Bounds: the oracle takes powf, the program (float)pow((double)..) as the kernels do.  alpha = 1 makes every priority exact, so indices and
the whole tree are equal and only the weights (one pow each) differ: rtol 5e-6, the bound of tests/test_gpu_per.py.  alpha = 0.6: indices
equal, tree within rtol 3e-7 (that test's bound for the tree)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bdr_agent_group_set_prioritized"


# ------------------------------------------------------------------------------------------------ the symbol
def test_the_new_call_is_on_every_surface():
    from border_amd import DqnGroup, _lib, build
    lib = C.CDLL(build.build_library())
    assert hasattr(lib, NAME)
    assert NAME in _lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    assert re.search(rf"BDR_API int32_t {NAME}\(bdr_agent_group\* g, int32_t on\);", hdr)
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    assert re.search(rf"pub fn {NAME}\s*\(g: \*mut bdr_agent_group, on: i32\) -> i32;", ffi)
    group_rs = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
    assert f"ffi::{NAME}(" in group_rs and "pub fn set_prioritized(&mut self, on: bool)" in group_rs
    assert f"`{NAME}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in (DqnGroup.__init__, DqnGroup.build):
        assert inspect.signature(fn).parameters["prioritized"].default is False
    assert callable(DqnGroup.set_prioritized)


def test_a_null_group_is_refused():
    from border_amd import build
    lib = C.CDLL(build.build_library())
    fn = getattr(lib, NAME)
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int32], C.c_int32
    lib.bdr_last_error.restype = C.c_char_p
    for on in (0, 1, 7):
        assert fn(None, on) == 1   # BDR_ERR_INVALID
        assert b"null group" in lib.bdr_last_error()


# ------------------------------------------------------------------------------------------------ the program
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group_per") / "group_per_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "group_per_sim.cpp"), "-o", exe])
    return exe


def hexf(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


class Case:
    """A script for the program and, from the oracle, what it must print."""

    def __init__(self, capacity, normalize, alpha, seed):
        from oracle.oracle import SumTree
        self.c, self.alpha = capacity, alpha
        self.t = SumTree(capacity, alpha, normalize)
        self.rng = np.random.default_rng(seed)
        self.head, self.pushed = 0, 0
        self.lines, self.want = [], []
        self.max_overwritten = 0

    def push(self, n=1):
        for _ in range(n):
            tree = self.t.tree()
            leaves = tree[self.c - 1:]
            if self.pushed >= self.c and leaves[self.head] == leaves.max() and (leaves == leaves.max()).sum() == 1:
                self.max_overwritten += 1     # this push replaces the one leaf that holds the maximum
            self.t.add(self.head, self.t.max())
            self.head = (self.head + 1) % self.c
            self.pushed += 1
            self.lines.append("P")

    def sample(self, n, beta, edge=False):
        u = (self.rng.integers(0, 1 << 23, n).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
        if edge:
            u[0], u[1] = np.float32(0.0), np.float32(8388607.0 / 8388608.0)
        ixs, ws = self.t.sample(u, np.float32(beta))
        self.lines.append(f"S {n} {hexf(beta)} " + " ".join(hexf(x) for x in u))
        self.want.append(("S", ixs, ws))
        return ixs

    def update(self, ixs, big_at=None):
        td = np.abs(self.rng.standard_normal(len(ixs))).astype(np.float32)
        td[self.rng.random(len(ixs)) < 0.1] = 0.0
        if big_at is not None:
            ixs = np.array(ixs).copy()
            ixs[-1], td[-1] = big_at, np.float32(50.0)
        for ix, p in zip(ixs, td):
            self.t.update(int(ix), float(p))
        self.lines.append(f"U {len(ixs)} " + " ".join(f"{int(i)} {hexf(p)}" for i, p in zip(ixs, td)))

    def tree(self):
        self.lines.append("T")
        self.want.append(("T", self.t.tree()))

    def round(self, n, beta, edge=False, big_at=None):
        self.update(self.sample(n, beta, edge), big_at)
        self.tree()


def build_case(capacity, normalize, alpha):
    k = Case(capacity, normalize, alpha, 7 * capacity + (normalize == "Batch") + int(10 * alpha))
    c = capacity
    k.push(min(5, c - 1) if c > 2 else 1)          # a few rows: tree[right] == 0 all over the descent, every batch full of duplicates
    k.round(32, 0.4, edge=True)
    k.round(32, 0.55)
    if c // 2 > k.pushed:                           # half full
        k.push(c // 2 - k.pushed)
        k.round(32, 0.7, edge=True)
    k.push(c - k.pushed)                            # full, head back at 0
    k.round(32, 0.85)
    k.round(17, 1.0, edge=True, big_at=k.head)      # the head row becomes THE maximum leaf ...
    k.push(1)                                       # ... and this single-row push overwrites it
    k.tree()
    k.push(c // 3 + 3)                              # wrapped
    k.round(32, 1.0, big_at=k.head)
    k.push(2)
    k.round(32, 1.0, edge=True)
    return k


@pytest.mark.parametrize("alpha", [1.0, 0.6])
@pytest.mark.parametrize("normalize", ["All", "Batch"])
@pytest.mark.parametrize("capacity", [2, 3, 8, 37, 100, 700, 4097, 5000])
def test_the_grouped_schedules_give_the_reference_tree(sim, tmp_path, capacity, normalize, alpha):
    k = build_case(capacity, normalize, alpha)
    path = tmp_path / "script.txt"
    path.write_text("\n".join(k.lines) + "\n")
    res = subprocess.run([sim, str(capacity), "0" if normalize == "All" else "1", repr(alpha), str(path)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]     # (a sanitizer report ends the program with a non-zero status)
    got = res.stdout.splitlines()
    assert len(got) == len(k.want)
    n_dup = 0
    for line, want in zip(got, k.want):
        assert line[0] == want[0]
        if want[0] == "S":
            left, right = line[2:].split("|")
            ixs = np.array(left.split(), np.int64)
            ws = np.array([int(x, 16) for x in right.split()], np.uint32).view(np.float32)
            assert (ixs == want[1]).all(), (capacity, normalize, alpha)
            assert (ixs >= 0).all() and (ixs < capacity).all()
            n_dup += len(ixs) - len(set(ixs.tolist()))
            if alpha == 1.0:
                np.testing.assert_allclose(ws, want[2], rtol=5e-6, atol=0)   # (u = 0 may end on a never-set leaf: inf in both)
        else:
            tree = np.array([int(x, 16) for x in line[2:].split()], np.uint32).view(np.float32)
            assert tree.shape == want[1].shape == (2 * capacity - 1,)
            if alpha == 1.0:
                assert (tree.view(np.uint32) == want[1].view(np.uint32)).all(), (capacity, normalize)
            else:
                np.testing.assert_allclose(tree, want[1], rtol=3e-7, atol=0)
    # what the script is there for
    assert n_dup >= 26 * 2                      # twice 32 draws from at most 5 rows (and the never-set leaf u = 0 may end on)
    assert k.pushed > capacity                  # wrapped
    assert k.max_overwritten >= 1               # a single-row push replaced the maximum leaf
    if capacity == 4097: assert 2 * capacity - 1 == 8191 + 2
