"""Reference <-> internal layout of the Nature-CNN trunk's six conv tensors (border_amd/csrc/conv_layout.hpp), on the host alone.

The tch DQN, IQN's psi and the candle DQN's AtariCnn form all convert c1 / c2 / c3 through conv_to_internal and conv_to_reference.
The header has no HIP in it: it is compiled here with the host compiler into a program of its own, run on ref[i] = i (every value
below 2^24: exact in f32, every element distinct), and its arena is compared bit for bit with the layout written out in numpy.

The same header holds the plan of the conv layers' weight-gradient partials (conv_dw_plan): a second program prints it, and the
test pins the buffer layout, the chunk counts of a batch and every per-layer item the kernels' callers read from it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "conv_layout.hpp"
// argv: n_stack internal.bin roundtrip.bin;  stdout: the two returned counts, the arena's offsets w1 b1 w2 b2 w3 b3 and the conv floats (w4)
static int dump(const char* path, const std::vector<float>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f) return 1;
    const size_t n = fwrite(v.data(), sizeof(float), v.size(), f);
    return (fclose(f) != 0 || n != v.size()) ? 1 : 0;
}
int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int ns = atoi(argv[1]);
    const bdr::Arena ar = bdr::make_arena(1, ns);
    std::vector<float> ref(bdr::conv_ref_floats(ns)), in(ar.w4, -1.f), back(ref.size(), -1.f);
    for (size_t i = 0; i < ref.size(); ++i) ref[i] = (float)i;
    const size_t n_in = bdr::conv_to_internal(ar, ref.data(), in.data());
    const size_t n_back = bdr::conv_to_reference(ar, in.data(), back.data());
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", n_in, n_back, ar.w1, ar.b1, ar.w2, ar.b2, ar.w3, ar.b3, ar.w4);
    return dump(argv[2], in) + dump(argv[3], back);
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("conv_layout")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "conv_layout"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe), d


def expected_arena(ref, ns, off, total, swap_khkw=False):
    """The internal arena written out in numpy: W1 [64 ns][32], W2 [(kh, kw, c)][o], W3 [(kh, kw, c)][o], the biases copied; each
    tensor at the offset make_arena reports.  swap_khkw: the (wrong) layout with kh and kw exchanged, for the mutation check."""
    t = (3, 2, 1, 0) if swap_khkw else (2, 3, 1, 0)
    sizes = [2048 * ns, 32, 32768, 64, 36864, 64]
    c1w, c1b, c2w, c2b, c3w, c3b = np.split(ref, np.cumsum(sizes)[:-1])
    parts = [c1w.reshape(32, 64 * ns).T, c1b, c2w.reshape(64, 32, 4, 4).transpose(*t).reshape(512, 64), c2b,
             c3w.reshape(64, 64, 3, 3).transpose(*t).reshape(576, 64), c3b]
    out = np.full(total, -1.0, np.float32)   # (the program's fill: the segments have no padding between them, so none of it survives)
    for o, p in zip(off, parts):
        out[o:o + p.size] = np.ascontiguousarray(p).ravel()
    return out


@pytest.mark.parametrize("ns", [1, 4])   # 1: the smallest; 4: every benchmark's
def test_conv_layout_round_trips_and_matches_the_numpy_layout(prog, ns):
    exe, d = prog
    f_in, f_back = str(d / f"in{ns}.bin"), str(d / f"back{ns}.bin")
    out = subprocess.run([exe, str(ns), f_in, f_back], capture_output=True, text=True, check=True).stdout.split()
    n_in, n_back, *off, total = map(int, out)
    n_ref = 2048 * ns + 32 + 32768 + 64 + 36864 + 64
    ref = np.arange(n_ref, dtype=np.float32)
    assert n_ref < 2 ** 24 and (ref.astype(np.int64) == np.arange(n_ref)).all()
    # round trip: the identity, and both calls report the reference floats they walked
    assert n_in == n_ref and n_back == n_ref
    back = np.fromfile(f_back, np.float32)
    assert back.size == n_ref and back.tobytes() == ref.tobytes()
    # the arena against the layout written out independently, bit for bit
    arena = np.fromfile(f_in, np.float32)
    assert arena.size == total
    assert off == list(np.cumsum([0, 2048 * ns, 32, 32768, 64, 36864])) and total == n_ref   # every segment a multiple of 4 floats: no padding
    assert arena.tobytes() == expected_arena(ref, ns, off, total).tobytes()
    # mutation check: kh and kw exchanged is a different arena, in W2 and in W3, so the comparison above can tell the layouts apart
    wrong = expected_arena(ref, ns, off, total, swap_khkw=True)
    assert arena.tobytes() != wrong.tobytes()
    for k in (2, 4):
        seg = slice(off[k], off[k + 1])
        assert (arena[seg] != wrong[seg]).any()
    for k in (0, 1, 3, 5):
        seg = slice(off[k], off[k + 1] if k < 5 else total)
        assert (arena[seg] == wrong[seg]).all()


# ---- the plan of the conv layers' weight-gradient partials (conv_dw_plan) ------------------------------------------------------------
PLAN_MAIN = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "conv_layout.hpp"
// argv: capacity n_stack;  stdout: "total w1 w2 w3" (the plan's total, make_arena's offsets), one line per layer
// "off stride allocated n n_weights w scale_bits wgs", then one line "Bn c1 c2 c3" of chunks(Bn) for every 1 <= Bn <= capacity
int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const int B = atoi(argv[1]), ns = atoi(argv[2]);
    const bdr::Arena ar = bdr::make_arena(6, ns);
    const bdr::ConvDwPlan p = bdr::conv_dw_plan(ar, B);
    printf("%zu %zu %zu %zu\n", p.total, ar.w1, ar.w2, ar.w3);
    for (const bdr::ConvDwLayer& l : p.layer) {
        uint32_t bits;
        memcpy(&bits, &l.wscale, 4);
        printf("%zu %zu %d %d %d %zu %u %d\n", l.off, l.stride, l.allocated, l.n, l.n_weights, l.w, bits, l.wgs);
    }
    for (int Bn = 1; Bn <= B; ++Bn) printf("%d %d %d %d\n", Bn, p.layer[0].chunks(Bn), p.layer[1].chunks(Bn), p.layer[2].chunks(Bn));
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("conv_dw_plan")
    src = d / "main.cpp"
    src.write_text(PLAN_MAIN)
    exe = d / "conv_dw_plan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


# (capacity, n_stack, BDR_DW_CHUNKS) -> allocated chunks, offsets, total, {Bn: chunks(Bn)}; None: not pinned for that case.
# The literals are the former dw_plan's: min(256, B), min(64, ceil(81 B / 32)), min(56, ceil(49 B / 32)), each capped by
# BDR_DW_CHUNKS; strides 2048 ns + 32, 32832, 36928; conv1's partials first, then conv2's, then conv3's.
PLAN_CASES = [
    (1, 4, None, (1, 3, 2), (0, 8224, 106720), 180576, {}),
    (2, 1, None, (2, 6, 4), (0, 4160, 201152), 348864, {}),
    (40, 4, None, (40, 64, 56), (0, 328960, 2430208), 4498176, {40: (40, 64, 56)}),
    (65, 4, None, (65, 64, 56), (0, 534560, 2635808), 4703776, {5: (5, 13, 8)}),   # a batch below the capacity: layout by capacity, chunks by batch
    (257, 4, None, (256, 64, 56), None, None, {257: (256, 64, 56)}),
    (40, 4, "4,8,16", (4, 8, 16), (0, 32896, 295552), 886400, {}),
]


@pytest.mark.parametrize("cap,ns,env,alloc,offs,total,filled", PLAN_CASES, ids=[f"B{c[0]}_ns{c[1]}" + ("_capped" if c[2] else "") for c in PLAN_CASES])
def test_conv_dw_plan_lays_out_the_partials_and_counts_the_filled_chunks(plan_prog, cap, ns, env, alloc, offs, total, filled):
    e = {k: v for k, v in os.environ.items() if k != "BDR_DW_CHUNKS"}
    if env:
        e["BDR_DW_CHUNKS"] = env
    lines = subprocess.run([plan_prog, str(cap), str(ns)], capture_output=True, text=True, check=True, env=e).stdout.splitlines()
    p_total, w1, w2, w3 = map(int, lines[0].split())
    layers = [tuple(map(int, ln.split())) for ln in lines[1:4]]
    chunks = {int(ln.split()[0]): tuple(map(int, ln.split()[1:])) for ln in lines[4:]}
    off, stride, allocated, n, n_weights, w, scale_bits, wgs = map(list, zip(*layers))
    assert tuple(allocated) == alloc
    if offs is not None:
        assert tuple(off) == offs and p_total == total
    for bn, c in filled.items():
        assert chunks[bn] == c
    # the three regions are disjoint, in the order conv1, conv2, conv3, and end at the total
    assert off[0] == 0 and off[1] == off[0] + allocated[0] * stride[0] and off[2] == off[1] + allocated[1] * stride[1]
    assert p_total == off[2] + allocated[2] * stride[2]
    # no batch up to the capacity fills more chunks than the buffer holds (and every batch fills at least one)
    assert sorted(chunks) == list(range(1, cap + 1))
    assert all(1 <= c[k] <= allocated[k] for c in chunks.values() for k in range(3))
    assert n == stride and stride == [2048 * ns + 32, 512 * 64 + 64, 576 * 64 + 64]
    assert n_weights == [2048 * ns, 32768, 36864]
    assert w == [w1, w2, w3] and w == [0, 2048 * ns + 32, 2048 * ns + 32 + 32768 + 64]
    one, inv255 = np.float32(1.0), np.float32(1.0) / np.float32(255.0)
    assert scale_bits == [int(inv255.view(np.uint32)), int(one.view(np.uint32)), int(one.view(np.uint32))]
    assert wgs == [1, 8, 9]
