"""Reference <-> internal layout of the Nature-CNN trunk's six conv tensors (border_amd/csrc/conv_layout.hpp), on the host alone.

The tch DQN, IQN's psi and the candle DQN's AtariCnn form all convert c1 / c2 / c3 through conv_to_internal and conv_to_reference.
The header has no HIP in it: it is compiled here with the host compiler into a program of its own, run on ref[i] = i (every value
below 2^24: exact in f32, every element distinct), and its arena is compared bit for bit with the layout written out in numpy."""
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
