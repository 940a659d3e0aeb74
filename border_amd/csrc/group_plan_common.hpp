// ================================================================================================
// What the launch plans of the agent groups share (bc_group_plan.hpp, iql_group_plan.hpp, awac_group_plan.hpp, group_layers_plan.hpp), without HIP in it:
// the hardware limits of a launch, the row chunks of the grouped weight gradient, the gather's workgroups per row, and the refusals of
// a group that do not depend on the kind of its members.  The plan headers keep their own names (bg_*, ig_*, ag_*, gl_*) as forwarders.
#pragma once
#include <algorithm>
#include <cstdint>
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

}  // namespace bdr
