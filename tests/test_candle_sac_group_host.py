"""The rule of a candle SAC group on the host alone (border_amd/csrc/candle_sac_group_plan.hpp): which agents may form a group, and
the launches of one update round.  The header has no HIP in it: it is compiled here with the host compiler into a program of its own.
Its plan is checked against a restatement, written here, of the launches Sac::opt_ enqueues for one member (candle_sac.hip
CandleSac::update and sample_logp, candle_actor.hpp actor_step / critic_step, dense_agent.hpp mlp_forward / mlp_backward_step, dense.hpp
dense_dx_z, replay.hip replay_sample_on_stream) with the member index as grid dimension y and the network instance as grid dimension
z.  Header, _lib.py and ffi.rs are checked on the new symbols."""
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
#include "candle_sac_group_plan.hpp"

using namespace bdr;

static int net_of(char** a, int in, int out_dim, CsNet& n)   // activation_out n_units units... -> arguments read
{
    n = CsNet{};
    n.activation_out = atoi(a[0]);
    const int nu = atoi(a[1]);
    for (int i = 0; i <= nu && i < CS_SHAPE_LAYERS; ++i) {
        const int out = i < nu ? atoi(a[2 + i]) : out_dim;
        n.Kp[i] = (in + 63) / 64 * 64; n.Np[i] = (out + 63) / 64 * 64; n.out[i] = out;
        in = out;
    }
    n.n_layers = nu + 1;
    return 2 + nu;
}
static int shape_of(char** a, CsShape& s)   // obs act batch n_critics actor_kind <critic net> <actor net> -> arguments read
{
    s = CsShape{};
    s.obs_dim = atoi(a[0]); s.act_dim = atoi(a[1]); s.batch = atoi(a[2]); s.n_critics = atoi(a[3]); s.actor_kind = atoi(a[4]);
    int at = 5;
    at += net_of(a + at, s.obs_dim + s.act_dim, 1, s.critic);
    at += net_of(a + at, s.obs_dim, s.actor_kind == CS_ACTOR_MLP2 ? 2 * s.act_dim : s.act_dim, s.actor);
    return at;
}

// plan P <shape>            -> count, every launch
// refuse n <member>...      member: kind_csac n_updates device prof grad_comm id <shape> ';'
// many P <shape>            -> the refusal of P identical members with distinct ids
int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "plan")) {
        const unsigned P = (unsigned)atoi(argv[2]);
        CsShape s;
        shape_of(argv + 3, s);
        const char* why = cs_shape_ineligible(s);
        if (why) printf("why %s\n", why);
        printf("count %d\n", cs_launch_count(s.critic.n_layers, s.actor.n_layers));
        printf("dense %d\n", cs_dense_launches(s.critic.n_layers, s.actor.n_layers));
        printf("lanes %d\n", cs_sample_lanes(s.act_dim));
        CsLaunch plan[CS_MAX_LAUNCHES];
        const int n = cs_round_plan(s, P, plan);
        if (n > CS_MAX_LAUNCHES) return 3;
        for (int i = 0; i < n; ++i)
            printf("launch %d %d %d %u %u %u %u %d %s\n", plan[i].kernel, plan[i].net, plan[i].layer, plan[i].gx, plan[i].gy, plan[i].gz, plan[i].threads,
                   cs_grid_ok(plan[i]) ? 1 : 0, cs_kernel_name(plan[i].kernel));
        return 0;
    }
    std::vector<CsMember> ms;
    if (!strcmp(argv[1], "refuse")) {
        int at = 3;
        for (int p = 0; p < atoi(argv[2]); ++p) {
            CsMember m{};
            m.kind_csac = atoi(argv[at]); m.n_updates = (uint64_t)atoi(argv[at + 1]); m.device = atoi(argv[at + 2]); m.prof = atoi(argv[at + 3]);
            m.grad_comm = atoi(argv[at + 4]); m.agent = (const void*)(size_t)atoi(argv[at + 5]);
            at += 6;
            at += shape_of(argv + at, m.shape);
            if (at >= argc || strcmp(argv[at], ";")) return 2;
            ++at;
            ms.push_back(m);
        }
    } else if (!strcmp(argv[1], "many")) {
        CsMember m{};
        m.kind_csac = 1; m.n_updates = 1;
        shape_of(argv + 3, m.shape);
        for (long p = 0; p < atol(argv[2]); ++p) { m.agent = (const void*)(size_t)(p + 1); ms.push_back(m); }
    } else return 2;
    const char* why = "";
    int kernel = -1;
    const int who = cs_group_refusal(ms.data(), (unsigned)ms.size(), &why, &kernel);
    printf("who %d\n", who);
    if (who != CS_OK) printf("why %s\n", why);
    if (kernel >= 0) printf("kernel %s\n", cs_kernel_name(kernel));
    return 0;
}
"""

KERNELS = ("gather", "pack", "fwd", "dx", "sample_logp", "alpha", "qmin", "actor_grad", "critic_loss", "dw", "reduce_adam")   # CsKernel's order
NETS = {-1: None, 0: "actor", 1: "critic"}
ACT = {"None": 0, "ReLU": 1}
KIND = {"Mlp3": 0, "Mlp2": 1}
# (obs, act, critic units, actor units, critic activation_out, actor kind, NC, B): the shapes of tests/test_gpu_candle_sac_group.py
SHAPES = {
    "partial_block": (17, 6, (64, 48), (64, 48), "None", "Mlp2", 2, 7),
    "pen": (45, 24, (256, 256), (256, 256), "None", "Mlp2", 2, 41),
    "no_hidden": (9, 4, (), (64,), "ReLU", "Mlp3", 1, 33),
    "wide_action": (21, 70, (64, 64, 64), (128,), "None", "Mlp3", 2, 20),
    "one_action": (3, 1, (64, 64), (64, 64), "None", "Mlp2", 2, 34),
}
PEN_BENCH = (45, 24, (256, 256), (256, 256), "None", "Mlp2", 2, 256)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("candle_sac_group")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "candle_sac_group"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def with_(shape, nc=None, batch=None, critic=None, actor=None, act_out=None, kind=None, act=None):
    od, ad, qu, pu, ao, ak, NC, B = shape
    return (od, ad if act is None else act, qu if critic is None else critic, pu if actor is None else actor, ao if act_out is None else act_out,
            ak if kind is None else kind, NC if nc is None else nc, B if batch is None else batch)


def shape_args(shape, **kw):
    od, ad, qu, pu, ao, ak, NC, B = with_(shape, **kw)
    out = [od, ad, B, NC, KIND[ak]]
    out += [ACT[ao], len(qu)] + list(qu) + [0, len(pu)] + list(pu)
    return [str(x) for x in out]


def run(prog, args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = {"launches": [], "grid_ok": [], "names": []}
    for line in r.stdout.splitlines():
        k, rest = line.split(" ", 1)
        if k == "launch":
            kern, net, layer, gx, gy, gz, th, ok, name = rest.split(" ", 8)
            out["launches"].append((KERNELS[int(kern)], NETS[int(net)], int(layer), int(gx), int(gy), int(gz), int(th)))
            out["grid_ok"].append(ok == "1")
            out["names"].append(name)
        else:
            out[k] = rest
    return out


def pad64(x):
    return (x + 63) // 64 * 64


def lanes(ad):
    """CandleSac::sample_logp: lanes per row, the smallest power of two that holds act_dim, at most 64"""
    G = 1
    while G < ad and G < 64:
        G *= 2
    return G


def launches(shape, P):
    """what Sac::opt_ enqueues for one member (CandleSac::update behind the gather), with P as grid y and the network instance as grid z"""
    od, ad, qu, pu, _ao, ak, NC, B = shape
    RB = (B + 31) // 32
    mlp2 = ak == "Mlp2"

    def net(i, units, o):
        w = [i] + list(units) + [o]
        return [pad64(x) for x in w[:-1]], [pad64(x) for x in w[1:]]
    nets = {"critic": net(od + ad, qu, 1), "actor": net(od, pu, 2 * ad if mlp2 else ad)}
    chunks = max(1, min(16, B // 256))

    def fwd(name, nz):   # mlp_forward: dense_forward_z per layer, k_dense_small with the instance in z
        Kp, Np = nets[name]
        return [("fwd", name, i, RB * (Np[i] // 32), P, nz, 256) for i in range(len(Np))]

    def dx(name, nz, lo):   # dense_dx_z (small) of layers L - 1 .. lo
        Kp, Np = nets[name]
        return [("dx", name, i, RB * (Kp[i] // 32), P, nz, 256) for i in range(len(Np) - 1, lo - 1, -1)]

    def step(name, nz, extra=0):   # mlp_backward_step: dX down to layer 1, ONE grouped dW over nz x L jobs, reduce + Adam with z = instance
        Kp, Np = nets[name]
        L = len(Np)
        out = dx(name, nz, 1)
        out.append(("dw", name, -1, nz * sum((Kp[i] // 32) * (Np[i] // 32) * chunks for i in range(L)), P, 1, 256))
        total = sum(Kp[i] * Np[i] + Np[i] for i in range(L)) + extra
        out.append(("reduce_adam", name, -1, (total // 4 + 255) // 256, P, nz, 256))
        return out

    def sample(draw):    # sample_logp: k_csac_sample_logp, 256 / G rows per workgroup
        rows = 256 // lanes(ad)
        return [("sample_logp", "actor", draw, (B + rows - 1) // rows, P, 1, 256)]
    nvec = od * 4 // 16 if od * 4 % 16 == 0 else od
    out = [("gather", None, -1, B * max(1, (nvec + 1023) // 1024), P, 1, 256), ("pack", None, -1, min((B * (od + ad) + 255) // 256, 2048), P, 1, 256)]
    # update_actor: the actor on obs, a + logp + partials, alpha, the online critics on (obs | act) and (obs | a), qmin, the critics' input
    # gradients down to the input layer, the actor's gradient (A + 1 workgroups), actor_step (head2 is Mlp3's)
    out += fwd("actor", 1) + sample(0) + [("alpha", None, -1, 1, P, 1, 1024)] + fwd("critic", 2 * NC)
    out += [("qmin", "critic", -1, (B + 255) // 256, P, 1, 256)] + dx("critic", NC, 0)
    out += [("actor_grad", "actor", -1, ad + 1, P, 1, 1024)] + step("actor", 1, 0 if mlp2 else pad64(ad))
    # update_critic: the updated actor on next_obs, next_a + logp, the target critics, the loss, critic_step
    out += fwd("actor", 1) + sample(1) + fwd("critic", NC) + [("critic_loss", "critic", -1, 1, P, 1, 1024)] + step("critic", NC)
    return out


def check_plan(prog, s, P):
    got = run(prog, ["plan", P] + shape_args(s))
    want = launches(s, P)
    Lq, Lp = len(s[2]) + 1, len(s[3]) + 1
    assert got["launches"] == want, s
    assert got["count"] == str(3 * Lp + 4 * Lq + 10) and len(want) == int(got["count"])
    assert int(got["dense"]) == sum(1 for l in want if l[0] in ("fwd", "dx")) == 3 * Lp + 4 * Lq - 2
    assert all(got["grid_ok"]) and all(l[4] == P for l in got["launches"])   # the member index is grid y of every launch
    assert all(l[5] <= 4 for l in got["launches"])                           # at most four instances
    return got


@pytest.mark.parametrize("P", [1, 8])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_plan_is_sac_opts_launch_list_for_every_member(prog, name, P):
    for nc in (1, 2):
        for kind in ("Mlp2", "Mlp3"):
            s = with_(SHAPES[name], nc=nc, kind=kind)
            if kind == "Mlp2" and len(s[3]) < 2:
                s = with_(s, actor=(128, 96))   # an Mlp2 trunk has at least two layers (unequal depth against a (64, 64, 64) critic stays unequal)
            check_plan(prog, s, P)


@pytest.mark.parametrize("act,G,rows", [(1, 1, 256), (6, 8, 32), (24, 32, 8), (70, 64, 4)])
def test_lanes_per_row_of_sample_logp(prog, act, G, rows):
    for B in (7, 41, 256, 300):
        for P in (1, 8):
            s = with_(SHAPES["pen"], act=act, batch=B)
            got = check_plan(prog, s, P)
            assert got["lanes"] == str(G) and lanes(act) == G
            sl = [l for l in got["launches"] if l[0] == "sample_logp"]
            assert [l[2] for l in sl] == [0, 1] and all(l[3] == (B + rows - 1) // rows for l in sl)
            assert [l for l in got["launches"] if l[0] == "actor_grad"] == [("actor_grad", "actor", -1, act + 1, P, 1, 1024)]


def test_pen_round(prog):
    got = run(prog, ["plan", 8] + shape_args(PEN_BENCH))
    assert got["count"] == "31" and len(got["launches"]) == 31     # the standalone update's 30 launches behind the gather
    kinds = [l[0] for l in got["launches"]]
    assert kinds == (["gather", "pack"] + ["fwd"] * 3 + ["sample_logp", "alpha"] + ["fwd"] * 3 + ["qmin"] + ["dx"] * 3 + ["actor_grad"] + ["dx"] * 2 +
                     ["dw", "reduce_adam"] + ["fwd"] * 3 + ["sample_logp"] + ["fwd"] * 3 + ["critic_loss"] + ["dx"] * 2 + ["dw", "reduce_adam"])
    assert got["launches"][7] == ("fwd", "critic", 0, 8 * 8, 8, 4, 256)
    assert got["launches"][5] == ("sample_logp", "actor", 0, 32, 8, 1, 256) and got["launches"][14] == ("actor_grad", "actor", -1, 25, 8, 1, 1024)
    # the critics' input-gradient chain: z = NC, down to the input layer (Kp = pad64(45 + 24) = 128)
    assert got["launches"][11:14] == [("dx", "critic", 2, 8 * 8, 8, 2, 256), ("dx", "critic", 1, 8 * 8, 8, 2, 256), ("dx", "critic", 0, 8 * 4, 8, 2, 256)]
    ra = [l for l in got["launches"] if l[0] == "reduce_adam"]
    assert [(l[1], l[5]) for l in ra] == [("actor", 1), ("critic", 2)]
    # the Mlp2 actor's arena has no head2: 64 x 256 + 256 + 256 x 256 + 256 + 256 x 64 + 64 floats
    assert ra[0][3] == ((64 * 256 + 256 + 256 * 256 + 256 + 256 * 64 + 64) // 4 + 255) // 256
    assert got["names"][2] == "k_dense_small_members_z<fwd>" and got["names"][5] == "k_csac_sample_logp_group" and got["names"][6] == "k_csac_alpha_group"
    assert got["names"][10] == "k_csac_qmin_group" and got["names"][14] == "k_csac_actor_grad_group" and got["names"][-1] == "k_csac_reduce_adam_group"
    assert got["launches"][-1][1] == "critic"                      # the critics' reduce + Adam is the round's last launch: it publishes


def test_a_critic_without_hidden_layers_has_the_unmasked_input_layer_alone(prog):
    got = run(prog, ["plan", 3] + shape_args(SHAPES["no_hidden"]))
    # dq/da is the input layer's dX alone (z = NC = 1); the critics' step has no dX; the actor's step has one
    assert [l for l in got["launches"] if l[0] == "dx"] == [("dx", "critic", 0, 2 * 2, 3, 1, 256), ("dx", "actor", 1, 2 * 2, 3, 1, 256)]
    assert got["count"] == str(3 * 2 + 4 * 1 + 10)
    assert [l for l in got["launches"] if l[0] == "fwd" and l[1] == "critic"] == [("fwd", "critic", 0, 2 * 2, 3, 2, 256), ("fwd", "critic", 0, 2 * 2, 3, 1, 256)]


def member(shape, kind_csac=1, n_updates=1, device=0, prof=0, grad_comm=0, ident=1, **kw):
    return [kind_csac, n_updates, device, prof, grad_comm, ident] + shape_args(shape, **kw) + [";"]


def refusal(prog, members):
    return run(prog, ["refuse", len(members)] + [x for m in members for x in m])


def test_every_refusal_names_the_first_member_concerned(prog):
    s = SHAPES["partial_block"]
    ok = lambda i: member(s, ident=i)
    assert refusal(prog, [ok(1), ok(2), ok(3)])["who"] == "-1"
    cases = {
        "not a candle SAC agent": member(s, kind_csac=0, ident=9),
        "differs from member 0's": member(s, ident=9, critic=(64, 64)),            # another shape (same padded widths)
        "one shape per group": member(s, ident=9, batch=8),
        "shape (obs_dim": member(SHAPES["pen"], ident=9),
        "activation_out": member(s, ident=9, act_out="ReLU"),
        "actor_kind": member(s, ident=9, kind="Mlp3"),                             # another actor kind
        "n_critics, batch_size": member(s, ident=9, nc=1),
        "n_critics > 2": member(s, ident=9, nc=3),
        "16 jobs": member(s, ident=9, critic=(64,) * 8),                           # 2 x 9 weight-gradient jobs
        "segments": member(s, ident=9, kind="Mlp3", actor=(64,) * 11),             # 12 layers + head2
        "segments (12": member(s, ident=9, actor=(64,) * 12),                      # an Mlp2 actor of 13 layers
        "head2 is one more": member(s, ident=9, nc=1, critic=(64,) * 12),          # 13 critic layers
        "n_updates_per_opt": member(s, ident=9, n_updates=2),
        "profiling": member(s, ident=9, prof=1),
        "gradient communicator": member(s, ident=9, grad_comm=1),
        "another device": member(s, ident=9, device=1),
        "earlier member already": ok(2),
    }
    for text, bad in cases.items():
        got = refusal(prog, [ok(1), ok(2), bad, ok(4)])
        assert got["who"] == "2" and text in got["why"], (text, got)
    # an Mlp2 actor of 12 layers has 12 segments and is no reason; the same depth as Mlp3 has 13
    twelve = lambda i, kind: member(s, ident=i, kind=kind, actor=(64,) * 11)
    assert refusal(prog, [twelve(1, "Mlp2"), twelve(2, "Mlp2")])["who"] == "-1"
    got = refusal(prog, [twelve(1, "Mlp3"), twelve(2, "Mlp3")])
    assert got["who"] == "0" and "segments" in got["why"]
    # member 0 itself can be the one
    got = refusal(prog, [member(s, nc=3, ident=1), ok(2)])
    assert got["who"] == "0" and "n_critics > 2" in got["why"]
    got = refusal(prog, [member(s, n_updates=4, ident=1)])
    assert got["who"] == "0" and "n_updates_per_opt" in got["why"]


def test_the_shape_checks_all_dense_kinds_share_keep_their_texts_and_their_order(prog):
    """gp_shape_ineligible (group_plan_common.hpp): the four texts that are the same for the IQL, AWAC and candle SAC groups, and where
    the kind's own reasons rank among them - the layer counts, the actor kind, n_critics, the 2 n_critics launch, the weight-gradient
    jobs, the reduce segments, the batch size, the dims"""
    s = SHAPES["partial_block"]

    def why(raw_kind=None, obs=None, **kw):
        a = shape_args(s, **kw)
        if obs is not None: a[0] = str(obs)
        if raw_kind is not None: a[4] = str(raw_kind)
        got = run(prog, ["plan", 2] + a)
        assert ("why" in got) == (not got["launches"])   # a shape with a reason has no plan
        return got.get("why")
    deep, jobs, segs = dict(critic=(64,) * 16), dict(critic=(64,) * 8), dict(actor=(64,) * 12)   # 17 layers; 2 x 9 jobs; 13 segments
    assert why() is None
    assert why(**deep) == "a network has no layer, or more than 16"
    assert why(nc=0) == "n_critics must be positive"
    assert why(**jobs) == "n_critics x critic layers beyond the 16 jobs of one grouped weight-gradient launch"
    assert why(obs=0) == "bad obs/act dims" and why(act=0) == "bad obs/act dims"
    # two reasons at once: the earlier one is named
    assert why(raw_kind=7, **deep) == "a network has no layer, or more than 16"
    assert why(raw_kind=7, nc=0) == "unknown actor kind"
    assert why(nc=0, **jobs) == "n_critics must be positive"
    assert why(nc=3, **jobs).startswith("n_critics > 2")
    assert "16 jobs" in why(**jobs, **segs)
    assert "segments (12" in why(batch=1, **segs)
    assert "at least 2 rows" in why(batch=1, obs=0)


def test_group_size_and_launch_limits(prog):
    s = SHAPES["partial_block"]
    assert run(prog, ["many", 65535] + shape_args(s))["who"] == "-1"
    for n in (0, 65536):
        got = run(prog, ["many", n] + shape_args(s))
        assert got["who"] == "-2" and "65535 members" in got["why"]
    got = run(prog, ["plan", 65535] + shape_args(s))
    assert all(got["grid_ok"])
    for kern, _net, _layer, gx, gy, gz, th in got["launches"]:
        assert 1 <= gx < 2**31 and gy == 65535 and 1 <= gz <= 4 and gx * gy * gz * th < 2**32, kern
    names = {"dw": "k_dense_dw_small_members", "gather": "k_gather_group", "fwd": "k_dense_small_members_z<fwd>", "dx": "k_dense_small_members_z<dx>",
             "sample_logp": "k_csac_sample_logp_group", "actor_grad": "k_csac_actor_grad_group", "pack": "k_csac_pack_group", "alpha": "k_csac_alpha_group",
             "qmin": "k_csac_qmin_group", "critic_loss": "k_csac_critic_loss_group", "reduce_adam": "k_csac_reduce_adam_group"}
    # 65535 members of the pen shape at batch 256 still fit: the online critics' first layer (8 x 8 tiles x 4 instances x 65535 x 256 threads
    # = (2^16 - 1) 2^16), the gather (256 x 65535 x 256) and the critics' grouped weight gradient (2 x 112 tiles) stay below 2^32 threads
    assert run(prog, ["many", 65535] + shape_args(PEN_BENCH))["who"] == "-1"
    assert all(l[3] * l[4] * l[5] * l[6] < 2**32 for l in launches(PEN_BENCH, 65535))
    # beyond it the refusal names the first launch of the restated round that does not fit: the gather at batch 512, the critics' grouped
    # weight gradient (2 x 176 tiles) with one more hidden layer
    first = {}
    for key, shape in (("batch", with_(PEN_BENCH, batch=512)), ("rows", with_(PEN_BENCH, batch=4096)), ("deep", with_(PEN_BENCH, critic=(256, 256, 256)))):
        plan = run(prog, ["plan", 65535] + shape_args(shape))
        bad = [(l[0], l[1]) for l, ok in zip(plan["launches"], plan["grid_ok"]) if not ok]
        want_bad = [(l[0], l[1]) for l in launches(shape, 65535) if l[3] * l[4] * l[5] * l[6] >= 2**32]
        assert bad and bad == want_bad
        got = run(prog, ["many", 65535] + shape_args(shape))
        assert got["who"] == "-2" and "2^32 threads" in got["why"] and got["kernel"] == names[bad[0][0]]
        first[key] = got["kernel"]
    assert first["batch"] == "k_gather_group" and first["deep"] == "k_dense_dw_small_members"
    # act_dim 255 at batch 64 with narrow networks: the actor gradient's (A + 1) x P x 1024 threads is the launch that does not fit
    wide = (45, 255, (64,), (64, 64), "None", "Mlp3", 2, 64)
    plan = run(prog, ["plan", 65535] + shape_args(wide))
    bad = [l[0] for l, ok in zip(plan["launches"], plan["grid_ok"]) if not ok]
    got = run(prog, ["many", 65535] + shape_args(wide))
    assert got["who"] == "-2" and got["kernel"] == names[bad[0]] and "actor_grad" in bad
    assert run(prog, ["many", 4096] + shape_args(PEN_BENCH))["who"] == "-1"


NEW = tuple("bdr_candle_sac_group_" + n for n in ("create", "destroy", "size", "member", "info", "opt", "opt_with_scalars", "sync", "sample", "sample_members"))
NEW_VOID = tuple("bdr_candle_sac_group_" + n for n in ("eval_ops_default", "trainer_ops_default", "trainer_post_default"))


def test_header_lib_py_and_ffi_rs_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    lib_py = open(os.path.join(ROOT, "border_amd", "_lib.py")).read()
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    for name in NEW + NEW_VOID:
        ret = "void" if name in NEW_VOID else "int32_t"
        decl = re.search(r"BDR_API %s %s\(([^;]*)\);[ \t]*/\*([^\n]*)\*/" % (ret, name), header)
        assert decl, name
        assert "sac/base.rs" in decl.group(2), name                   # every declaration cites the reference's agent
        n_args = len(decl.group(1).split(","))
        assert '"%s"' % name in lib_py, name
        types = re.search(r"L\.%s\.argtypes = \[(.*)\]" % name, lib_py)
        assert types and len(types.group(1).split(",")) == n_args, name
        rust = re.search(r"pub fn %s\(([^;]*)\)%s;" % (name, "" if name in NEW_VOID else " -> i32"), ffi)
        assert rust and len([a for a in rust.group(1).split(",") if a.strip()]) == n_args, name
    m = re.search(r"#define BDR_GROUP_FORM_CANDLE_SAC_LAYERS (\d+)", header)
    assert m and m.group(1) == "5" and re.search(r"pub const BDR_GROUP_FORM_CANDLE_SAC_LAYERS: i32 = %s;" % m.group(1), ffi)
    forms = re.search(r"GROUP_FORM_CANDLE_SAC_LAYERS = (\d+)", lib_py)
    assert forms and forms.group(1) == m.group(1)
    assert "pub enum bdr_candle_sac_group {}" in ffi and "typedef struct bdr_candle_sac_group bdr_candle_sac_group;" in header
    group_py = open(os.path.join(ROOT, "border_amd", "group.py")).read()
    assert "class CandleSacGroup(_DenseGroup)" in group_py and '"bdr_candle_sac_group"' in group_py and '"candle_sac_layers"' in group_py
    assert 'RECORD_KEYS = ("loss_critic", "loss_actor", "ent_coef")' in group_py
    assert "pub struct AmdCandleSacGroup" in open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
