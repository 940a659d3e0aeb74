"""The rule of a candle DQN group on the host alone (border_amd/csrc/candle_dqn_group_plan.hpp): which agents may form a group, and
the launches of one update round.  The header has no HIP in it: it is compiled here with the host compiler into a program of its own.
Its plan is checked against a restatement, written here, of the launches Dqn::opt_ enqueues for one member (candle_dqn.hip
CandleDqn::opt / update, dense_agent.hpp mlp_forward / mlp_backward_step, replay.hip replay_sample_on_stream) with the member index as
grid dimension y and the network instance of a forward launch as grid dimension z.  Header, _lib.py and ffi.rs are checked on the new
symbols."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "candle_dqn_group_plan.hpp"

using namespace bdr;

// obs actions batch double_dqn form activation_out n_units units... -> arguments read
static int shape_of(char** a, CqShape& s)
{
    s = CqShape{};
    s.obs_dim = atoi(a[0]); s.n_actions = atoi(a[1]); s.batch = atoi(a[2]); s.double_dqn = atoi(a[3]); s.form = atoi(a[4]);
    s.net.activation_out = atoi(a[5]);
    const int nu = atoi(a[6]);
    int in = s.obs_dim;
    for (int i = 0; i <= nu && i < CQ_SHAPE_LAYERS; ++i) {
        const int out = i < nu ? atoi(a[7 + i]) : s.n_actions;
        s.net.Kp[i] = (in + 63) / 64 * 64; s.net.Np[i] = (out + 63) / 64 * 64; s.net.out[i] = out;
        in = out;
    }
    s.net.n_layers = nu + 1;
    return 7 + nu;
}

// plan P <shape>            -> count, every launch
// refuse n <member>...      member: kind_cdqn n_updates device prof grad_comm id <shape> ';'
// many P <shape>            -> the refusal of P identical members with distinct ids
int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "plan")) {
        const unsigned P = (unsigned)atoi(argv[2]);
        CqShape s;
        shape_of(argv + 3, s);
        const char* why = cq_shape_ineligible(s);
        if (why) printf("why %s\n", why);
        printf("count %d\n", cq_launch_count(s.net.n_layers));
        printf("dense %d\n", cq_dense_launches(s.net.n_layers));
        CqLaunch plan[CQ_MAX_LAUNCHES];
        const int n = cq_round_plan(s, P, plan);
        if (n > CQ_MAX_LAUNCHES) return 3;
        for (int i = 0; i < n; ++i)
            printf("launch %d %d %d %u %u %u %u %d %s\n", plan[i].kernel, plan[i].net, plan[i].layer, plan[i].gx, plan[i].gy, plan[i].gz, plan[i].threads,
                   cq_grid_ok(plan[i]) ? 1 : 0, cq_kernel_name(plan[i].kernel));
        return 0;
    }
    std::vector<CqMember> ms;
    if (!strcmp(argv[1], "refuse")) {
        int at = 3;
        for (int p = 0; p < atoi(argv[2]); ++p) {
            CqMember m{};
            m.kind_cdqn = atoi(argv[at]); m.n_updates = (uint64_t)atoi(argv[at + 1]); m.device = atoi(argv[at + 2]); m.prof = atoi(argv[at + 3]);
            m.grad_comm = atoi(argv[at + 4]); m.agent = (const void*)(size_t)atoi(argv[at + 5]);
            at += 6;
            at += shape_of(argv + at, m.shape);
            if (at >= argc || strcmp(argv[at], ";")) return 2;
            ++at;
            ms.push_back(m);
        }
    } else if (!strcmp(argv[1], "many")) {
        CqMember m{};
        m.kind_cdqn = 1; m.n_updates = 1;
        shape_of(argv + 3, m.shape);
        for (long p = 0; p < atol(argv[2]); ++p) { m.agent = (const void*)(size_t)(p + 1); ms.push_back(m); }
    } else return 2;
    const char* why = "";
    int kernel = -1;
    const int who = cq_group_refusal(ms.data(), (unsigned)ms.size(), &why, &kernel);
    printf("who %d\n", who);
    if (who != CQ_OK) printf("why %s\n", why);
    if (kernel >= 0) printf("kernel %s\n", cq_kernel_name(kernel));
    return 0;
}
"""

KERNELS = ("gather", "pack", "fwd", "dx", "td", "dw", "reduce_adam")   # CqKernel's order
NAMES = {"gather": "k_gather_group", "pack": "k_cdqn_pack_group", "fwd": "k_dense_small_members_z<fwd>", "dx": "k_dense_small_members_z<dx>",
         "td": "k_cdqn_td_group", "dw": "k_dense_dw_small_members", "reduce_adam": "k_cdqn_reduce_adam_group"}
ACT = {"None": 0, "ReLU": 1}
# (obs, actions, units, batch, double_dqn, activation_out): the shapes of tests/test_gpu_candle_dqn_group.py
SHAPES = {
    "cartpole_small": (4, 2, (64, 64), 64, False, "None"),
    "odd_double": (70, 33, (128,), 37, True, "None"),
    "no_hidden": (9, 5, (), 33, False, "None"),
    "seven_layers": (6, 3, (64,) * 6, 16, True, "None"),
    "relu_out": (4, 2, (64, 64), 64, False, "ReLU"),
}
DQN_CARTPOLE = (4, 2, (256, 256), 64, False, "None")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("candle_dqn_group")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "candle_dqn_group"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def with_(shape, obs=None, actions=None, units=None, batch=None, double=None, act_out=None):
    od, A, u, B, dd, ao = shape
    return (od if obs is None else obs, A if actions is None else actions, u if units is None else units, B if batch is None else batch,
            dd if double is None else double, ao if act_out is None else act_out)


def shape_args(shape, form=0, **kw):
    od, A, u, B, dd, ao = with_(shape, **kw)
    return [str(x) for x in [od, A, B, int(dd), form, ACT[ao], len(u)] + list(u)]


def run(prog, args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = {"launches": [], "grid_ok": [], "names": []}
    for line in r.stdout.splitlines():
        k, rest = line.split(" ", 1)
        if k == "launch":
            kern, net, layer, gx, gy, gz, th, ok, name = rest.split(" ", 8)
            out["launches"].append((KERNELS[int(kern)], int(net), int(layer), int(gx), int(gy), int(gz), int(th)))
            out["grid_ok"].append(ok == "1")
            out["names"].append(name)
        else:
            out[k] = rest
    return out


def pad64(x):
    return (x + 63) // 64 * 64


def launches(shape, P):
    """what Dqn::opt_ enqueues for one member (CandleDqn::opt: the gather, then CandleDqn::update), with P as grid y and the network
    instance of a forward launch as grid z"""
    od, A, units, B, dd, _ao = shape
    RB = (B + 31) // 32
    w = [od] + list(units) + [A]
    Kp, Np = [pad64(x) for x in w[:-1]], [pad64(x) for x in w[1:]]
    L = len(Np)
    chunks = max(1, min(16, B // 256))
    nvec = od * 4 // 16 if od * 4 % 16 == 0 else od
    out = [("gather", -1, -1, B * max(1, (nvec + 1023) // 1024), P, 1, 256)]            # replay_sample_on_stream
    out.append(("pack", -1, -1, (B * od + 255) // 256, P, 1, 256))                      # k_cdqn_pack: one thread per element of [B][O]
    # mlp_forward: (p, obs), (p_tgt, next_obs) and - double_dqn - (p, next_obs) share each layer's launch
    out += [("fwd", 0, i, RB * (Np[i] // 32), P, 3 if dd else 2, 256) for i in range(L)]
    out.append(("td", 0, -1, 1, P, 1, 1024))                                            # k_cdqn_td: ONE 1024-thread workgroup
    # mlp_backward_step from the last layer: dX down to layer 1, ONE grouped dW, reduce + Adam over the arena
    out += [("dx", 0, i, RB * (Kp[i] // 32), P, 1, 256) for i in range(L - 1, 0, -1)]
    out.append(("dw", 0, -1, sum((Kp[i] // 32) * (Np[i] // 32) * chunks for i in range(L)), P, 1, 256))
    total = sum(Kp[i] * Np[i] + Np[i] for i in range(L))
    out.append(("reduce_adam", 0, -1, (total // 4 + 255) // 256, P, 1, 256))
    return out


def check_plan(prog, s, P):
    got = run(prog, ["plan", P] + shape_args(s))
    want = launches(s, P)
    L = len(s[2]) + 1
    assert got["launches"] == want, s
    assert got["count"] == str(2 * L + 4) and len(want) == 2 * L + 4
    assert int(got["dense"]) == sum(1 for l in want if l[0] in ("fwd", "dx")) == 2 * L - 1
    assert all(got["grid_ok"]) and all(l[4] == P for l in got["launches"])   # the member index is grid y of every launch
    assert got["names"] == [NAMES[l[0]] for l in want]
    return got


@pytest.mark.parametrize("P", [1, 5, 64])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_plan_is_dqn_opts_launch_list_for_every_member(prog, name, P):
    for dd in (False, True):
        for B in (SHAPES[name][3], 300, 1024):
            check_plan(prog, with_(SHAPES[name], double=dd, batch=B), P)


def test_dqn_cartpole_round(prog):
    got = check_plan(prog, DQN_CARTPOLE, 8)
    assert got["count"] == "10"                        # the standalone update's 9 launches behind the gather
    assert [l[0] for l in got["launches"]] == ["gather", "pack", "fwd", "fwd", "fwd", "td", "dx", "dx", "dw", "reduce_adam"]
    assert got["launches"][2] == ("fwd", 0, 0, 2 * 8, 8, 2, 256) and got["launches"][5] == ("td", 0, -1, 1, 8, 1, 1024)
    assert got["launches"][-1][0] == "reduce_adam"     # the round's last launch: it publishes
    # double DQN: a third instance in every forward launch and nowhere else
    dd = check_plan(prog, with_(DQN_CARTPOLE, double=True), 8)
    assert [l[5] for l in dd["launches"]] == [1, 1, 3, 3, 3, 1, 1, 1, 1, 1]


def test_no_hidden_layer_has_no_input_gradient(prog):
    got = check_plan(prog, SHAPES["no_hidden"], 3)
    assert got["count"] == "6" and not [l for l in got["launches"] if l[0] == "dx"]


def member(shape, kind_cdqn=1, n_updates=1, device=0, prof=0, grad_comm=0, ident=1, form=0, **kw):
    return [kind_cdqn, n_updates, device, prof, grad_comm, ident] + shape_args(shape, form=form, **kw) + [";"]


def refusal(prog, members):
    return run(prog, ["refuse", len(members)] + [x for m in members for x in m])


def test_every_refusal_names_the_first_member_concerned(prog):
    s = SHAPES["cartpole_small"]
    ok = lambda i: member(s, ident=i)
    assert refusal(prog, [ok(1), ok(2), ok(3)])["who"] == "-1"
    cases = {
        "not a candle DQN agent": member(s, kind_cdqn=0, ident=9),
        "AtariCnn": member(s, ident=9, form=1),
        "n_updates_per_opt": member(s, ident=9, n_updates=2),
        "differs from member 0's": member(s, ident=9, units=(64, 48)),             # another shape (same padded widths)
        "one shape per group": member(s, ident=9, batch=65),
        "shape (obs_dim": member(s, ident=9, obs=5),
        "n_actions": member(s, ident=9, actions=3),
        "activation_out": member(s, ident=9, act_out="ReLU"),
        "double_dqn": member(s, ident=9, double=True),
        "12 segments": member(s, ident=9, units=(64,) * 12),                       # 13 layers
        "weight-gradient launch (16)": member(s, ident=9, units=(64,) * 15),       # 16 layers: beyond the reduce segments
        "profiling": member(s, ident=9, prof=1),
        "gradient communicator": member(s, ident=9, grad_comm=1),
        "another device": member(s, ident=9, device=1),
        "earlier member already": ok(2),
    }
    for text, bad in cases.items():
        got = refusal(prog, [ok(1), ok(2), bad, ok(4)])
        assert got["who"] == "2" and text in got["why"], (text, got)
    # 12 layers fit both launches; member 0 itself can be the one refused
    twelve = lambda i: member(s, ident=i, units=(64,) * 11)
    assert refusal(prog, [twelve(1), twelve(2)])["who"] == "-1"
    got = refusal(prog, [member(s, ident=1, form=1), ok(2)])
    assert got["who"] == "0" and "AtariCnn" in got["why"]
    got = refusal(prog, [member(s, n_updates=4, ident=1)])
    assert got["who"] == "0" and "n_updates_per_opt" in got["why"]
    for kw in (dict(batch=0), dict(batch=65537), dict(obs=0), dict(actions=0), dict(actions=4097)):
        got = run(prog, ["plan", 2] + shape_args(s, **kw))
        assert "why" in got and not got["launches"], kw


def test_group_size_and_launch_limits(prog):
    s = SHAPES["cartpole_small"]
    assert run(prog, ["many", 65535] + shape_args(s))["who"] == "-1"
    for n in (0, 65536):
        got = run(prog, ["many", n] + shape_args(s))
        assert got["who"] == "-2" and "65535 members" in got["why"]
    got = run(prog, ["plan", 65535] + shape_args(DQN_CARTPOLE))
    assert all(got["grid_ok"])
    for kern, _net, _layer, gx, gy, gz, th in got["launches"]:
        assert 1 <= gx < 2**31 and gy == 65535 and 1 <= gz <= 3 and gx * gy * gz * th < 2**32, kern
    # beyond the limits the refusal names the first launch of the restated round that does not fit
    first = {}
    for key, shape in (("batch", with_(DQN_CARTPOLE, batch=512)), ("wide", with_(DQN_CARTPOLE, units=(2048,), double=True)),
                       ("deep", with_(DQN_CARTPOLE, units=(256,) * 5))):
        plan = run(prog, ["plan", 65535] + shape_args(shape))
        bad = [l[0] for l, ok in zip(plan["launches"], plan["grid_ok"]) if not ok]
        want_bad = [l[0] for l in launches(shape, 65535) if l[3] * l[4] * l[5] * l[6] >= 2**32]
        assert bad and bad == want_bad, key
        got = run(prog, ["many", 65535] + shape_args(shape))
        assert got["who"] == "-2" and "2^32 threads" in got["why"] and got["kernel"] == NAMES[bad[0]], key
        first[key] = got["kernel"]
    assert first["batch"] == "k_gather_group" and first["wide"] == "k_dense_small_members_z<fwd>" and first["deep"] == "k_dense_dw_small_members"
    assert run(prog, ["many", 4096] + shape_args(with_(DQN_CARTPOLE, batch=512)))["who"] == "-1"


NEW = tuple("bdr_candle_dqn_group_" + n for n in ("create", "destroy", "size", "member", "info", "opt", "opt_with_scalars", "sync", "sample", "sample_members",
                                                  "last_q", "push", "push_max_rows"))
NEW_VOID = tuple("bdr_candle_dqn_group_" + n for n in ("eval_ops_default", "trainer_ops_default", "trainer_post_default"))


def test_header_lib_py_and_ffi_rs_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "border_amd", "_lib.py")).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    for name in NEW + NEW_VOID:
        ret = "void" if name in NEW_VOID else "int32_t"
        decl = re.search(r"BDR_API %s %s\(([^;]*)\);[ \t]*/\*([^\n]*)\*/" % (ret, name), header)
        assert decl, name
        assert ".rs:" in decl.group(2), name                           # every declaration cites the reference lines it restates
        n_args = len(decl.group(1).split(","))
        assert '"%s"' % name in lib_py, name
        types = re.search(r"L\.%s\.argtypes = \[(.*)\]" % name, lib_py)
        assert types and len(types.group(1).split(",")) == n_args, name
        rust = re.search(r"pub fn %s\(([^;]*)\)%s;" % (name, "" if name in NEW_VOID else " -> i32"), ffi)
        assert rust and len([a for a in rust.group(1).split(",") if a.strip()]) == n_args, name
    m = re.search(r"#define BDR_GROUP_FORM_CANDLE_DQN_LAYERS (\d+)", header)
    assert m and m.group(1) == "6" and re.search(r"pub const BDR_GROUP_FORM_CANDLE_DQN_LAYERS: i32 = %s;" % m.group(1), ffi)
    forms = re.search(r"GROUP_FORM_CANDLE_DQN_LAYERS = (\d+)", lib_py)
    assert forms and forms.group(1) == m.group(1)
    assert "pub enum bdr_candle_dqn_group {}" in ffi and "typedef struct bdr_candle_dqn_group bdr_candle_dqn_group;" in header
    group_py = open(os.path.join(ROOT, "border_amd", "group.py")).read()
    assert "class CandleDqnGroup(_GroupBase)" in group_py and '"bdr_candle_dqn_group"' in group_py and '"candle_dqn_layers"' in group_py
    assert "pub struct AmdCandleDqnGroup" in open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
    import border_amd
    assert border_amd.CandleDqnGroup.__name__ == "CandleDqnGroup"
