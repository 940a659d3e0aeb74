// ================================================================================================
// What the launch plans of the agent groups share (bc_group_plan.hpp, iql_group_plan.hpp, awac_group_plan.hpp, candle_sac_group_plan.hpp,
// group_layers_plan.hpp), without HIP in it: the hardware limits of a launch, the row chunks of the grouped weight gradient, the gather's
// workgroups per row, and the refusals of a group that do not depend on the kind of its members.  Below them, what the dense rounds share
// (the IQL, AWAC and candle SAC groups, whose launches have network instances): the launch, the limits and kernel ids of the shared
// launches, the plan writer, the common shape checks and the members' own refusals.
#pragma once
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>

namespace bdr {

constexpr unsigned GP_MAX_MEMBERS = 65535;   // the member index is grid dimension y
constexpr int GP_OK = -1, GP_NO_MEMBER = -2;

// hardware limits of a launch: 2^31 - 1 workgroups along x, 65535 along y and z, and (HIP) fewer than 2^32 threads in all
template <class Launch>
inline bool gp_grid_ok(const Launch& l)
{
    if (l.gx < 1 || l.gy < 1 || l.gz < 1 || l.gx > 0x7fffffffu || l.gy > 65535u || l.gz > 65535u) return false;
    return (uint64_t)l.gx * l.gy * l.gz * l.threads < (1ull << 32);
}
// row chunks of the grouped weight gradient (DenseAgent::chunks_for, DqnMlp::ensure_batch): 256 batch rows per workgroup, at most 16
inline int gp_dw_chunks(int batch) { const int c = batch / 256; return c < 1 ? 1 : (c > 16 ? 16 : c); }
// workgroups per sampled row of the gather: replay_gather_shape's rule (replay.hip) without its diagnostics override BDR_GATHER_CHUNKS -
// creating a BC or an IQL group compares the two and refuses the group while the override makes them differ, so the grid
// replay_gather_group launches is always the grid checked against the limits here
inline unsigned gp_gather_chunks(uint64_t obs_bytes)
{
    const uint64_t nvec = obs_bytes % 16 == 0 ? obs_bytes / 16 : obs_bytes / 4;
    const uint64_t c = (nvec + 1023) / 1024;
    return (unsigned)(c < 1 ? 1 : c);
}

// one Mlp as the plans of the candle-family groups (iql_group_plan.hpp, awac_group_plan.hpp) read it: padded sizes (multiples of 64:
// make_mlp) and logical output width of every layer, and whether its output has a ReLU
constexpr int GP_SHAPE_LAYERS = 16;
struct GpNet { int n_layers; int Kp[GP_SHAPE_LAYERS], Np[GP_SHAPE_LAYERS], out[GP_SHAPE_LAYERS]; int activation_out; };
inline bool gp_same_net(const GpNet& a, const GpNet& b)
{
    if (a.n_layers != b.n_layers || a.activation_out != b.activation_out) return false;
    for (int i = 0; i < a.n_layers && i < GP_SHAPE_LAYERS; ++i) if (a.Kp[i] != b.Kp[i] || a.Np[i] != b.Np[i] || a.out[i] != b.out[i]) return false;
    return true;
}
inline uint64_t gp_arena_floats(const GpNet& n)
{
    uint64_t total = 0;
    for (int i = 0; i < n.n_layers; ++i) total += (uint64_t)n.Kp[i] * n.Np[i] + n.Np[i];
    return total;
}
// tiles of the grouped weight gradient of one instance of the network
inline unsigned gp_dw_tiles(const GpNet& n, int batch)
{
    unsigned dw = 0;
    for (int i = 0; i < n.n_layers; ++i) dw += (unsigned)((n.Kp[i] / 32) * (n.Np[i] / 32) * gp_dw_chunks(batch));
    return dw;
}

// the first member that is the same agent as an earlier member (n: there is none); a sort, not n^2 / 2 comparisons at 65535 members
template <class Member>
inline unsigned gp_first_duplicate(const Member* m, unsigned n)
{
    std::vector<std::pair<const void*, unsigned>> v(n);
    for (unsigned p = 0; p < n; ++p) v[p] = {m[p].agent, p};
    std::sort(v.begin(), v.end());   // (equal agents in member order)
    unsigned first = n;
    for (unsigned i = 1; i < n; ++i) if (v[i].first == v[i - 1].first) first = std::min(first, v[i].second);
    return first;
}

// what the member-independent refusals read of a member
struct GpMember { int device, prof, grad_comm; const void* agent; };

// May these n agents form a group?  GP_OK: yes.  Otherwise *why says so; the return value is the first member the reason names, or
// GP_NO_MEMBER where it concerns the group as a whole (its size, a launch beyond the limits: *kernel names that launch).  For a member
// the kind's own reasons (`own(m[p])`: its shape, nullptr where it has none) win over the common ones: profiling, a gradient
// communicator, another device, a duplicate.  `plan(out)`: the launches of a round of n members of member 0's shape.
template <class Launch, int MAX_LAUNCHES, class Member, class Own, class Plan>
inline int gp_group_refusal(const Member* m, unsigned n, const char** why, int* kernel, Own own, Plan plan)
{
    if (kernel) *kernel = -1;
    if (n < 1 || n > GP_MAX_MEMBERS) { *why = "a group has 1 .. 65535 members"; return GP_NO_MEMBER; }
    const unsigned dup = gp_first_duplicate(m, n);
    for (unsigned p = 0; p < n; ++p) {
        const GpMember c{m[p].device, m[p].prof, m[p].grad_comm, m[p].agent};
        const char* w = own(m[p]);
        if (!w && c.prof) w = "profiling is on";
        if (!w && c.grad_comm) w = "a gradient communicator is installed";
        if (!w && c.device != m[0].device) w = "it lives on another device than member 0";
        if (!w && p == dup) w = "the same agent is an earlier member already";
        if (w) { *why = w; return (int)p; }
    }
    Launch l[MAX_LAUNCHES];
    const int nl = plan(l);
    for (int i = 0; i < nl; ++i)
        if (!gp_grid_ok(l[i])) {
            *why = "a launch of the round exceeds 2^31 - 1 / 65535 / 65535 workgroups or 2^32 threads";
            if (kernel) *kernel = l[i].kernel;
            return GP_NO_MEMBER;
        }
    return GP_OK;
}

// ---- the dense rounds: iql_group_plan.hpp, awac_group_plan.hpp, candle_sac_group_plan.hpp ---------------------------------------------
// limits of the shared launches (dense_group.hpp checks them against dense.hpp's): jobs of one grouped weight-gradient launch, segments
// of one reduce + Adam launch, instances of one dense or reduce + Adam launch
constexpr int GP_DW_GROUP = 16, GP_RA_SEGS = 12, GP_MAXZ = 4;
// net: the network a dense / dW / reduce / loss launch serves (the kind's net id, GP_NET_NONE: none), layer: the layer a forward / dX
// launch serves, the draw of a sample launch, else -1; gy = the members, gz = the instances nz of the launch
struct GpLaunch { int kernel, net, layer; unsigned gx, gy, gz, threads; };
constexpr int GP_NET_NONE = -1;
// The launches every dense round has.  The first four have one number in all kinds (pack is the kind's own entry under the shared
// id); a kind numbers its own launches from GP_K_OWN on and its weight gradient and reduce + Adam behind them, as its enum always
// has - the host tests mirror those numbers -, so the plan writer and the round (dense_group.hpp) take these two ids from the kind.
enum GpKernel { GP_K_GATHER = 0, GP_K_PACK, GP_K_FWD, GP_K_DX, GP_K_OWN };
// a pack kernel's grid (Iql / Awac / CandleSac::update): one thread per element of [B][width], at most 2048 workgroups (the body
// strides by the grid)
inline unsigned gp_pack_grid(int batch, int width)
{
    const uint64_t g = ((uint64_t)batch * (uint64_t)width + 255) / 256;
    return (unsigned)(g < 2048 ? g : 2048);
}

// Writes the launches of one round of P members at batch size B into `out`, in stream order: x is the member's own grid everywhere,
// y the member, z the network instance.  k_dw, k_reduce_adam: the kind's ids of the weight gradient and of reduce + Adam.
struct GpPlan {
    GpLaunch* out; int n; int B; unsigned P; int k_dw, k_reduce_adam;
    unsigned rb() const { return (unsigned)((B + 31) / 32); }
    // a launch of the kind's own, without instances
    void one(int kernel, int net, int layer, unsigned gx, unsigned threads) { out[n++] = GpLaunch{kernel, net, layer, gx, P, 1, threads}; }
    void gather(int obs_dim) { one(GP_K_GATHER, GP_NET_NONE, -1, (unsigned)B * gp_gather_chunks((uint64_t)obs_dim * 4), 256); }
    void pack(int width) { one(GP_K_PACK, GP_NET_NONE, -1, gp_pack_grid(B, width), 256); }
    // mlp_forward of nz instances of network `id`
    void fwd(const GpNet& net, int id, unsigned nz)
    {
        for (int i = 0; i < net.n_layers; ++i) out[n++] = GpLaunch{GP_K_FWD, id, i, rb() * (unsigned)(net.Np[i] / 32), P, nz, 256};
    }
    // the input gradients of the layers from the top down to `lo`
    void dx(const GpNet& net, int id, unsigned nz, int lo)
    {
        for (int i = net.n_layers - 1; i >= lo; --i) out[n++] = GpLaunch{GP_K_DX, id, i, rb() * (unsigned)(net.Kp[i] / 32), P, nz, 256};
    }
    // mlp_backward_step: the input gradients down to layer 1, the grouped weight gradient, reduce + Adam over `arena` floats
    void step(const GpNet& net, int id, unsigned nz, uint64_t arena)
    {
        dx(net, id, nz, 1);
        out[n++] = GpLaunch{k_dw, id, -1, nz * gp_dw_tiles(net, B), P, 1, 256};
        out[n++] = GpLaunch{k_reduce_adam, id, -1, (unsigned)((arena / 4 + 255) / 256), P, nz, 256};
    }
};

// Why an agent of a dense kind cannot be a member of any group (nullptr: it can): the checks all kinds share, in the precedence of the
// refusals.  The kind evaluates what is its own and hands it in: `first` (nullptr: passes) ranks behind the layer counts, `two_nc` is
// its text for more than GP_MAXZ / 2 critics, `segs` and `batch` (nullptr: passes) rank behind the weight-gradient jobs.
struct GpShapeOwn { const char *first, *two_nc, *segs, *batch; };
inline const char* gp_shape_ineligible(std::initializer_list<const GpNet*> nets, int n_critics, int critic_layers, int obs_dim, int act_dim, const GpShapeOwn& own)
{
    for (const GpNet* n : nets)
        if (n->n_layers < 1 || n->n_layers > GP_SHAPE_LAYERS) return "a network has no layer, or more than 16";
    if (own.first) return own.first;
    if (n_critics < 1) return "n_critics must be positive";
    if (2 * n_critics > GP_MAXZ) return own.two_nc;
    if (n_critics * critic_layers > GP_DW_GROUP) return "n_critics x critic layers beyond the 16 jobs of one grouped weight-gradient launch";
    if (own.segs) return own.segs;
    if (own.batch) return own.batch;
    if (obs_dim < 1 || act_dim < 1) return "bad obs/act dims";
    return nullptr;
}

// gp_group_refusal of a dense kind.  A member's own reasons, in their order: it is not of the kind (`is_kind` is the member's flag,
// `not_kind` the text), its shape is ineligible, its shape differs from member 0's (`shape_differs`), n_updates_per_opt.
template <int MAX_LAUNCHES, class Member, class Shape>
inline int gp_dense_group_refusal(const Member* m, unsigned n, const char** why, int* kernel, int Member::*is_kind, const char* not_kind, const char* shape_differs,
                                  const char* (*ineligible)(const Shape&), bool (*same_shape)(const Shape&, const Shape&),
                                  int (*round_plan)(const Shape&, unsigned, GpLaunch*))
{
    const auto own = [&](const Member& x) -> const char* {
        if (!(x.*is_kind)) return not_kind;
        if (const char* w = ineligible(x.shape)) return w;
        if (!same_shape(x.shape, m[0].shape)) return shape_differs;
        if (x.n_updates != 1) return "n_updates_per_opt != 1 is not built for a group";
        return nullptr;
    };
    return gp_group_refusal<GpLaunch, MAX_LAUNCHES>(m, n, why, kernel, own, [&](GpLaunch* out) { return round_plan(m[0].shape, n, out); });
}

}  // namespace bdr
