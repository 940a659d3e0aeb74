"""The rule of a BC group on the host alone (border_amd/csrc/bc_group_plan.hpp): which kernel form a BC agent takes, which agents may
form a group, and the launches of one update round.  The header has no HIP in it: it is compiled here with the host compiler into a
program of its own.  Its plan is checked against a restatement, written here, of the launches Bc::opt enqueues for one member
(bc.hip Bc::update, dense_agent.hpp mlp_forward / mlp_backward_step, replay.hip replay_sample_on_stream) with the member index as grid
dimension y."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bc_group_plan.hpp"

using namespace bdr;

static BgShape shape_of(char** a)   // obs act batch activation_out kernel_form action_type n_units units...
{
    BgShape s{};
    s.obs_dim = atoi(a[0]); s.act_dim = atoi(a[1]); s.batch = atoi(a[2]); s.activation_out = atoi(a[3]);
    const int nu = atoi(a[6]);
    s.form = bc_resolve_form(atoi(a[4]), s.batch, s.act_dim, nu); s.action_type = atoi(a[5]);
    int in = s.obs_dim;
    for (int i = 0; i <= nu && i < BG_SHAPE_LAYERS; ++i) {
        const int out = i < nu ? atoi(a[7 + i]) : s.act_dim;
        s.Kp[i] = (in + 63) / 64 * 64; s.Np[i] = (out + 63) / 64 * 64; s.out[i] = out;
        in = out;
    }
    s.n_layers = nu + 1;
    return s;
}

// plan P <shape>            -> form, count, every launch
// refuse n <member>...      member: device prof grad_comm id <shape> ';'
// many P <shape>            -> the refusal of P identical members with distinct ids
int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "plan")) {
        const unsigned P = (unsigned)atoi(argv[2]);
        const BgShape s = shape_of(argv + 3);
        const char* why = bg_shape_ineligible(s);
        printf("form %d\n", s.form);
        if (why) printf("why %s\n", why);
        printf("count %d\n", bg_launch_count(s.n_layers, s.form));
        BgLaunch plan[BG_MAX_LAUNCHES];
        const int n = bg_round_plan(s, P, plan);
        if (n > BG_MAX_LAUNCHES) return 3;
        for (int i = 0; i < n; ++i)
            printf("launch %d %d %u %u %u %u %d %s\n", plan[i].kernel, plan[i].layer, plan[i].gx, plan[i].gy, plan[i].gz, plan[i].threads, bg_grid_ok(plan[i]) ? 1 : 0,
                   bg_kernel_name(plan[i].kernel));
        return 0;
    }
    std::vector<BgMember> ms;
    if (!strcmp(argv[1], "refuse")) {
        int at = 3;
        for (int p = 0; p < atoi(argv[2]); ++p) {
            BgMember m{};
            m.device = atoi(argv[at]); m.prof = atoi(argv[at + 1]); m.grad_comm = atoi(argv[at + 2]); m.agent = (const void*)(size_t)atoi(argv[at + 3]);
            m.shape = shape_of(argv + at + 4);
            at += 4 + 7 + atoi(argv[at + 4 + 6]);
            if (at >= argc || strcmp(argv[at], ";")) return 2;
            ++at;
            ms.push_back(m);
        }
    } else if (!strcmp(argv[1], "many")) {
        BgMember m{};
        m.shape = shape_of(argv + 3);
        for (long p = 0; p < atol(argv[2]); ++p) { m.agent = (const void*)(size_t)(p + 1); ms.push_back(m); }
    } else return 2;
    const char* why = "";
    int kernel = -1;
    const int who = bg_group_refusal(ms.data(), (unsigned)ms.size(), &why, &kernel);
    printf("who %d\n", who);
    if (who != BG_OK) printf("why %s\n", why);
    if (kernel >= 0) printf("kernel %s\n", bg_kernel_name(kernel));
    return 0;
}
"""

KERNELS = ("gather", "pack", "fwd", "loss", "head", "dx", "dw", "reduce_adam")   # BgKernel's order
ACT = {"None": 0, "ReLU": 1, "Tanh": 2, "Sigmoid": 3}
FORMS = {"default": 0, "general": 1, "fused": 2, "fused_mfma": 3}
# the shapes of tests/test_gpu_bc_group.py, and bc_pen
SHAPES = {
    "partial_block": (17, 6, (64, 48), "None", 7),
    "two_blocks": (45, 24, (256, 256), "Tanh", 40),
    "head_nt2": (21, 40, (64,), "Sigmoid", 33),
    "no_hidden": (9, 4, (), "None", 20),
    "wide_out": (21, 65, (64, 40), "Tanh", 50),
    "bc_pen": (45, 24, (256, 256), "Tanh", 256),
}
HEAD_OK = ("partial_block", "two_blocks", "head_nt2", "bc_pen")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("bc_group")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "bc_group"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def shape_args(shape, form="general", action=1, units=None, batch=None):
    od, ad, un, act_out, bsz = shape
    un = un if units is None else units
    return [str(x) for x in (od, ad, bsz if batch is None else batch, ACT[act_out], FORMS[form], action, len(un)) + tuple(un)]


def run(prog, args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = {"launches": [], "grid_ok": []}
    for line in r.stdout.splitlines():
        k, rest = line.split(" ", 1)
        if k == "launch":
            kern, layer, gx, gy, gz, th, ok, _name = rest.split(" ", 7)
            out["launches"].append((KERNELS[int(kern)], int(layer), int(gx), int(gy), int(gz), int(th)))
            out["grid_ok"].append(ok == "1")
        else:
            out[k] = rest
    return out


def pad64(x):
    return (x + 63) // 64 * 64


def launches(shape, form, P):
    """what Bc::opt enqueues for one member, with P as grid y"""
    od, ad, units, _act_out, B = shape
    widths = [od] + list(units) + [ad]
    Kp, Np = [pad64(w) for w in widths[:-1]], [pad64(w) for w in widths[1:]]
    L, RB = len(Np), (B + 31) // 32
    head = form == "fused_mfma"
    nvec = od * 4 // 16 if od * 4 % 16 == 0 else od
    out = [("gather", -1, B * max(1, (nvec + 1023) // 1024), P, 1, 256), ("pack", -1, (B * od + 255) // 256, P, 1, 256)]
    out += [("fwd", i, RB * (Np[i] // 32), P, 1, 256) for i in range(L - 1 if head else L)]
    out.append(("head" if head else "loss", -1, RB, P, 1, 256))
    out += [("dx", i, RB * (Kp[i] // 32), P, 1, 256) for i in range(L - 2 if head else L - 1, 0, -1)]
    chunks = max(1, min(16, B // 256))
    out.append(("dw", -1, sum((Kp[i] // 32) * (Np[i] // 32) * chunks for i in range(L)), P, 1, 256))
    total = sum(Kp[i] * Np[i] + Np[i] for i in range(L))
    out.append(("reduce_adam", -1, (total // 4 + 255) // 256, P, 1, 256))
    return out


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_launch_counts(prog, L):
    units = (64,) * (L - 1)
    got = run(prog, ["plan", 3] + shape_args((17, 6, units, "None", 7), "general"))
    assert got["count"] == str(2 * L + 4) and len(got["launches"]) == 2 * L + 4
    if L >= 2:
        got = run(prog, ["plan", 3] + shape_args((17, 6, units, "None", 7), "fused_mfma"))
        assert got["count"] == str(2 * L + 2) and len(got["launches"]) == 2 * L + 2
    else:   # no hidden layer under the head: the count is the rule's, the shape is refused
        got = run(prog, ["plan", 3] + shape_args((17, 6, units, "None", 7), "fused_mfma"))
        assert got["count"] == "4" and got["launches"] == [] and "hidden layer" in got["why"]


@pytest.mark.parametrize("P", [1, 3, 1024])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_plan_is_bc_opts_launch_list_for_every_member(prog, name, P):
    for form in ("general", "fused_mfma") if name in HEAD_OK else ("general",):
        got = run(prog, ["plan", P] + shape_args(SHAPES[name], form))
        assert got["launches"] == launches(SHAPES[name], form, P), (name, form)
        assert all(got["grid_ok"]) and all(l[3] == P for l in got["launches"])   # the member index is grid y of every launch


def test_bc_pen_round(prog):
    got = run(prog, ["plan", 8] + shape_args(SHAPES["bc_pen"], "default"))
    assert got["form"] == "3"   # BDR_BC_KERNEL_DEFAULT resolves to the MFMA head at batch 256
    assert [l[0] for l in got["launches"]] == ["gather", "pack", "fwd", "fwd", "head", "dx", "dw", "reduce_adam"]
    assert got["launches"][4] == ("head", -1, 8, 8, 1, 256)
    assert got["launches"][6] == ("dw", -1, 2 * 8 + 8 * 8 + 8 * 2, 8, 1, 256)
    assert got["launches"][7] == ("reduce_adam", -1, ((64 * 256 + 256 + 256 * 256 + 256 + 256 * 64 + 64) // 4 + 255) // 256, 8, 1, 256)


def test_the_form_decision(prog):
    f = lambda shape, form, **kw: run(prog, ["plan", 1] + shape_args(shape, form, **kw))["form"]
    assert f(SHAPES["bc_pen"], "default") == "3" and f(SHAPES["bc_pen"], "default", batch=1024) == "3" and f(SHAPES["bc_pen"], "default", batch=1025) == "1"
    assert f(SHAPES["no_hidden"], "default") == "1" and f(SHAPES["wide_out"], "default") == "1"   # no hidden layer; act_dim > 64
    assert f(SHAPES["head_nt2"], "default") == "3" and f(SHAPES["bc_pen"], "fused") == "2" and f(SHAPES["bc_pen"], "general") == "1"


def member(shape, form="general", device=0, prof=0, grad_comm=0, ident=1, **kw):
    return [device, prof, grad_comm, ident] + shape_args(shape, form, **kw) + [";"]


def refusal(prog, members):
    return run(prog, ["refuse", len(members)] + [x for m in members for x in m])


def test_every_refusal_names_the_first_member_that_differs(prog):
    s = SHAPES["partial_block"]
    ok = lambda i: member(s, ident=i)
    assert refusal(prog, [ok(1), ok(2), ok(3)])["who"] == "-1"
    cases = {
        "differs from member 0": member(s, ident=9, units=(64, 64)),           # another shape (same padded widths)
        "differs from member 0's": member(s, ident=9, batch=8),
        "shape (obs_dim": member(SHAPES["two_blocks"], ident=9),
        "resolved kernel form": member(s, "fused_mfma", ident=9),
        "LDS head": member(s, "fused", ident=9),
        "Discrete": member(s, ident=9, action=0),
        "profiling": member(s, ident=9, prof=1),
        "gradient communicator": member(s, ident=9, grad_comm=1),
        "another device": member(s, ident=9, device=1),
        "earlier member already": ok(2),
        "more layers": member(s, ident=9, units=(64,) * 12),
    }
    for text, bad in cases.items():
        got = refusal(prog, [ok(1), ok(2), bad, ok(4)])
        assert got["who"] == "2" and text in got["why"], (text, got)
    # member 0 itself can be the one
    got = refusal(prog, [member(s, "fused", ident=1), ok(2)])
    assert got["who"] == "0" and "LDS head" in got["why"]
    got = refusal(prog, [member(SHAPES["wide_out"], "fused_mfma", ident=1)])
    assert got["who"] == "0" and "act_dim <= 64" in got["why"]


def test_of_two_duplicate_members_the_first_is_named(prog):
    """the duplicate search is a sort over (agent, member): it still names the FIRST member that repeats an earlier one"""
    s = SHAPES["partial_block"]
    got = refusal(prog, [member(s, ident=i) for i in (1, 2, 3, 2, 1)])   # member 3 repeats member 1, member 4 repeats member 0
    assert got["who"] == "3" and "earlier member already" in got["why"], got
    got = refusal(prog, [member(s, ident=i) for i in (1, 2, 3, 1, 2)])   # the same with the lower agent id at the later member
    assert got["who"] == "3" and "earlier member already" in got["why"], got


def test_group_size_and_launch_limits(prog):
    s = SHAPES["partial_block"]
    assert run(prog, ["many", 65535] + shape_args(s))["who"] == "-1"
    got = run(prog, ["many", 65536] + shape_args(s))
    assert got["who"] == "-2" and "65535 members" in got["why"]
    # every launch of 65535 members of the small shape, and of bc_pen, is within the limits; at batch 512 the gather is not: 512 x 65535
    # workgroups of 256 threads are 2^32 threads and more
    for shape, n in ((s, 10), (SHAPES["bc_pen"], 10)):
        got = run(prog, ["plan", 65535] + shape_args(shape))
        assert all(got["grid_ok"]) and len(got["launches"]) == n
        for kern, _layer, gx, gy, gz, th in got["launches"]:
            assert 1 <= gx < 2**31 and gy == 65535 and gz == 1 and gx * gy * gz * th < 2**32, kern
    plan = run(prog, ["plan", 65535] + shape_args(SHAPES["bc_pen"], batch=512))
    assert [l[0] for l, ok in zip(plan["launches"], plan["grid_ok"]) if not ok] == ["gather"]
    got = run(prog, ["many", 65535] + shape_args(SHAPES["bc_pen"], batch=512))
    assert got["who"] == "-2" and "2^32 threads" in got["why"] and got["kernel"] == "k_gather_group"
    assert run(prog, ["many", 65535] + shape_args(SHAPES["bc_pen"]))["who"] == "-1"
