"""The rule that classifies a member of an agent group and the launch plan of a layer-form round (border_amd/csrc/group_layers_plan.hpp),
on the host alone.  The header has no HIP in it: it is compiled here with the host compiler into a program of its own that prints, for
a shape and a number of members, the step the member takes and every launch of one round (kernel, grid, threads).  The output is
checked against tests/group_layers_restatement.py - a Python restatement of DqnMlp::fused_ok and of the launches update_critic
enqueues - for the shapes (a)-(d) of tests/test_gpu_group_layers.py and for C1, and every grid is checked against the launch limits
up to 1024 members."""
import os
import shutil
import subprocess

import pytest

from tests.group_layers_restatement import SHAPES, Shape, fused_ok, head_fused, launches

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "group_layers_plan.hpp"

// argv: P in_dim out_dim batch double_dqn small_gemm head_fuse n_units units...
int main(int argc, char** argv)
{
    if (argc < 9) return 2;
    const unsigned P = (unsigned)atoi(argv[1]);
    bdr::GlShape s{};
    s.in_dim = atoi(argv[2]); s.out_dim = atoi(argv[3]); s.batch = atoi(argv[4]); s.double_dqn = atoi(argv[5]);
    s.fused = 1; s.small_gemm = atoi(argv[6]); s.head_fuse = atoi(argv[7]);
    const int nu = atoi(argv[8]);
    if (argc != 9 + nu || nu + 1 > bdr::GL_SHAPE_LAYERS) return 2;
    int in = s.in_dim;
    for (int i = 0; i <= nu; ++i) {
        const int out = i < nu ? atoi(argv[9 + i]) : s.out_dim;
        s.Kp[i] = (in + 63) / 64 * 64; s.Np[i] = (out + 63) / 64 * 64;
        in = out;
    }
    s.n_layers = nu + 1;
    const bool fused = bdr::gl_fused_ok(s);
    const char* why = fused ? nullptr : bdr::gl_layers_ineligible(s);
    printf("form %s\n", fused ? "one_workgroup" : why ? "none" : "layers");
    if (why) printf("why %s\n", why);
    if (!fused && !why) printf("head %d\n", bdr::gl_head_fused(s) ? 1 : 0);
    bdr::GlLaunch plan[bdr::GL_MAX_LAUNCHES];
    const int n = bdr::gl_round_plan(s, P, plan);
    if (n > bdr::GL_MAX_LAUNCHES) return 3;
    for (int i = 0; i < n; ++i)
        printf("launch %d %d %u %u %u %u %d %s\n", plan[i].kernel, plan[i].layer, plan[i].gx, plan[i].gy, plan[i].gz, plan[i].threads, bdr::gl_grid_ok(plan[i]) ? 1 : 0,
               bdr::gl_kernel_name(plan[i].kernel));
    return 0;
}
"""

KERNELS = ("gather", "pack", "fwd", "head_td", "td_dense", "mean_rows", "dx", "dw", "reduce_adam", "step")   # GlKernel's order


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("group_layers")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "group_layers"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def plan_of(prog, s, P, small_gemm=1):
    r = subprocess.run([prog, str(P), str(s.in_dim), str(s.out_dim), str(s.batch), str(int(s.double_dqn)), str(small_gemm), str(int(s.head_fuse)),
                        str(len(s.units))] + [str(u) for u in s.units], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {"launches": []}
    for line in r.stdout.splitlines():
        k, rest = line.split(" ", 1)
        if k == "launch":
            kern, layer, gx, gy, gz, th, ok, _name = rest.split(" ", 7)
            out["launches"].append((KERNELS[int(kern)], int(gx), int(gy), int(gz), int(th)))
            out.setdefault("grid_ok", []).append(ok == "1")
        else:
            out[k] = rest
    return out


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
@pytest.mark.parametrize("P", [1, 3, 64, 1024])
def test_the_plan_is_update_critics_launch_list_for_every_member(prog, name, P):
    s = SHAPES[name]
    got = plan_of(prog, s, P)
    assert not fused_ok(s) and got["form"] == "layers"
    assert got["head"] == str(int(head_fused(s)))
    assert got["launches"] == launches(s, P)
    assert all(got["grid_ok"])
    assert len(got["launches"]) == {"a": 8, "b": 8, "c": 11, "d": 11}[name]   # the same number whatever P is


def test_the_reference_shape_is_eleven_launches(prog):
    """dqn_cartpole: gather, pack, three layers of two instances, TD rows, loss mean, two input gradients, 162 weight-gradient tiles
    (2 x 8 + 8 x 8 + 8 x 2 tiles of 32 x 32), reduce + Adam over 98 880 floats"""
    got = plan_of(prog, SHAPES["d"], 8)["launches"]
    assert [l[0] for l in got] == ["gather", "pack", "fwd", "fwd", "fwd", "td_dense", "mean_rows", "dx", "dx", "dw", "reduce_adam"]
    assert got[2] == ("fwd", 2 * 8, 8, 2, 256) and got[4] == ("fwd", 2 * 2, 8, 2, 256)
    assert got[9] == ("dw", 16 + 64 + 16, 8, 1, 256)
    assert got[10] == ("reduce_adam", (98880 // 4 + 255) // 256, 8, 1, 256)


def test_without_the_row_block_head(prog):
    s = Shape(4, (64, 64), 2, 65, head_fuse=False)
    got = plan_of(prog, s, 4)
    assert got["head"] == "0" and got["launches"] == launches(s, 4) and len(got["launches"]) == 11


@pytest.mark.parametrize("P", [1, 260])
def test_c1_and_smaller_take_the_one_workgroup_step(prog, P):
    for s in (SHAPES["c1"], Shape(4, (64, 64), 2, 32, double_dqn=True), Shape(3, (32,), 3, 17), Shape(6, (64, 32, 64), 5, 32)):
        got = plan_of(prog, s, P)
        assert fused_ok(s) and got["form"] == "one_workgroup"
        assert got["launches"] == [("step", P, 1, 1, 512)]


def test_the_fused_ok_rule_over_a_sweep_of_shapes(prog):
    """widths 32 .. 320, depth 1 .. 4, batch around the row-block edges, both DQN kinds: the header's rule equals the restatement's"""
    n = {"one_workgroup": 0, "layers": 0, "none": 0}
    for units in ((32,), (64,), (64, 64), (128, 64), (64, 128), (256, 256), (64, 192), (64, 64, 64), (64, 64, 64, 64), (320, 64), (64, 320)):
        for batch in (1, 32, 33, 64, 65, 128, 129):
            for ddqn in (False, True):
                s = Shape(4, units, 2, batch, double_dqn=ddqn)
                got = plan_of(prog, s, 2)
                want = "one_workgroup" if fused_ok(s) else "none" if (s.L > 4 or max(s.Kp + s.Np) > 256) else "layers"
                assert got["form"] == want, (units, batch, ddqn, got)
                n[want] += 1
                if want == "layers": assert got["launches"] == launches(s, 2)
                if want == "none": assert got["launches"] == [] and ("256" in got["why"] or "4 layers" in got["why"])
    assert min(n.values()) >= 10, n


def test_refusal_reasons(prog):
    assert "BDR_NO_SMALL_GEMM" in plan_of(prog, SHAPES["a"], 2, small_gemm=0)["why"]
    assert "wider than 256" in plan_of(prog, Shape(4, (320, 64), 2, 64), 2)["why"]
    assert "4 layers" in plan_of(prog, Shape(4, (64, 64, 64, 64), 2, 65), 2)["why"]


def test_grids_stay_within_the_launch_limits(prog):
    """every grid dimension of every launch for P = 1 .. 1024 (powers of two and their neighbours), widest and deepest eligible nets and
    the largest batch the replay layer hands out in one sample plan"""
    for s in (SHAPES["d"], Shape(64, (256, 256, 256), 32, 128), Shape(4, (64, 64), 2, 4096), Shape(256, (256, 256, 256), 64, 1000, double_dqn=True)):
        for P in sorted({p + d for p in (1, 2, 8, 64, 255, 256, 512, 1024) for d in (-1, 0, 1)} - {0, 1025}):
            got = plan_of(prog, s, P)
            assert got["form"] == "layers" and all(got["grid_ok"]), (s.units, P)
            for kern, gx, gy, gz, th in got["launches"]:
                assert 1 <= gx < 2**31 and 1 <= gy <= 65535 and 1 <= gz <= 65535 and gx * gy * gz * th < 2**32, (kern, gx, gy, gz)
                assert (gz if kern == "head_td" else gy) == P   # the member index is one grid dimension of every launch
