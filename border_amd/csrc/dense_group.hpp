// ================================================================================================
// The group entries of dense.hpp's generic kernels with the member as grid dimension y and the network instance as grid dimension z,
// for launch groupings whose launches have instances (iql_group.hpp: IQL; awac_group.hpp: AWAC; the end-of-round ticket the groupings share is group_done.hpp).
// Each entry runs the body of the kernel it groups on the member's entry of a device array, read in place through the constant address
// space: member and instance come from blockIdx, so they are uniform and the entry's fields are scalar loads, as they are from the
// kernel-argument segment of the standalone kernel.  Same bodies, same bits.  (BC's own entries, with one instance, stay in bc_group.hpp,
// which does not include this header.)
// Bounds: member = blockIdx.y < gridDim.y = P; launch i of the dense family is handed args + i * P, so it reads entry i * P + member of an
// array of (launches of the family) * P entries; z = blockIdx.z < gridDim.z = nz <= DG_MAXZ, the instances an entry holds.  Inside an
// instance every index is the body's own, with the bounds of the standalone kernel.
// The host half below writes those entries for one member: what mlp_forward / mlp_backward_step (dense_agent.hpp) hand the standalone
// launches of a network, for any kind whose member arguments hold `dense`, and `dw`, `dw_grid`, `ra` indexed by the kind's network id.
#pragma once
#include "dense.hpp"
#include "dense_agent.hpp"
#include "group_done.hpp"
#include "group_plan_common.hpp"

namespace {

constexpr int DG_MAXZ = 4;
static_assert(DG_MAXZ == RA_INST, "an entry holds the instances of one DenseArgsZ / ReduceAdamArgs launch");
// one member's arguments of one layer (or input-gradient) launch: instance z = blockIdx.z, as DenseArgsZ::a of the standalone launch
struct DenseGroupEntry { DenseArgs a[DG_MAXZ]; };

// a layer (DX = false) or an input gradient (DX = true) of every member's nz networks: grid (the member's own tiles, P, nz)
template <bool DX>
__global__ __launch_bounds__(256) void k_dense_small_members_z(const BDR_CONST_AS DenseGroupEntry* args)
{
    __shared__ float red[4][32][33];
    dense_small_body<DX>(args[blockIdx.y].a[blockIdx.z], red);
}
// the grouped weight gradient of every member: grid (the member's own dW tiles - all jobs of all its instances -, P)
__global__ __launch_bounds__(256) void k_dense_dw_small_members(const BDR_CONST_AS DenseDwSmallGroup* args) { dense_dw_small_group_body(args[blockIdx.y]); }

// a member's optimizer scalars of this step out of its staging slot: field by field (static indices, registers)
__device__ __forceinline__ AdamScalars dg_step_scalars(const BDR_CONST_AS AdamScalars& s)
{
    AdamScalars d;
    d.b1 = s.b1; d.omb1 = s.omb1; d.b2 = s.b2; d.omb2 = s.omb2; d.sqrt_bc2 = s.sqrt_bc2; d.eps = s.eps; d.neg_step = s.neg_step; d.wd_mul = s.wd_mul;
    return d;
}
// The body of a kind's reduce + Adam entry (awac_group.hpp, candle_sac_group.hpp), written once over the kind's per-step words: network
// NET of every member, instance z = blockIdx.z, the optimizer scalars from adam[NET] of the member's slot.  TRACK_LAST: the network
// tracks its targets at the member's own tau (a.tau / a.omt of its entry) and its launch is the last reader of the slot, which
// publishes (bg_group_done, behind a barrier every thread reaches: dense_reduce_adam_body returns to here, not out of the kernel).
// NET < the length of Step::adam is the kind's static_assert; member and z are bounded as above.
template <int NET, bool TRACK_LAST, class Step>
__device__ __forceinline__ void dg_reduce_adam_step(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS Step* steps, unsigned* ticket, unsigned* seq_host,
                                                    unsigned seq)
{
    const AdamScalars d = dg_step_scalars(steps[blockIdx.y].adam[NET]);
    dense_reduce_adam_body(args[blockIdx.y], (int)blockIdx.z, d, TRACK_LAST ? 1 : 0, 0);
    if constexpr (TRACK_LAST) bg_group_done(ticket, seq_host, seq);
}

// ---- host: one member's entries of the launches of one network (iql_group.hpp, awac_group.hpp, candle_sac_group.hpp) --------------------
// a network as the kinds' plan headers read it (group_plan_common.hpp)
inline GpNet dg_net_shape(const MlpLayout& net, int activation_out)
{
    GpNet s{};
    s.n_layers = (int)net.L.size(); s.activation_out = activation_out;
    for (int i = 0; i < s.n_layers && i < GP_SHAPE_LAYERS; ++i) { s.Kp[i] = net.L[i].Kp; s.Np[i] = net.L[i].Np; s.out[i] = net.L[i].out; }
    return s;
}
inline DenseArgs dg_fwd_args(const DenseLayer& l, const float* par, DenseSrc in, float* out, int bs)   // dense_forward_z
{
    DenseArgs d{};
    d.x = in; d.w = par + l.w; d.bias = par + l.b; d.out = out; d.ldo = l.Np;
    d.M = bs; d.ncols = l.Np; d.kred = l.Kp; d.relu = l.relu; d.w_ld = l.Np;
    return d;
}
inline DenseArgs dg_dx_args(const DenseLayer& l, const float* par, const float* dy, float* dx, const float* mask, int bs)   // dense_dx_z
{
    DenseArgs d{};
    d.x = DenseSrc{dy, l.Np}; d.w = par + l.w; d.out = dx; d.ldo = l.Kp; d.mask = mask; d.ldm = l.Kp;
    d.M = bs; d.ncols = l.Kp; d.kred = l.Np; d.w_ld = l.Np;
    return d;
}
// mlp_forward of nz (parameters, input, activations) triples of one architecture: one entry per layer
inline void dg_fwd_entries(std::vector<DenseGroupEntry>& out, const MlpLayout& net, int nz, const float* const* par, const float* const* x,
                           std::vector<float*>* const* acts, int bs)
{
    for (size_t l = 0; l < net.L.size(); ++l) {
        DenseGroupEntry e{};
        for (int z = 0; z < nz; ++z)
            e.a[z] = dg_fwd_args(net.L[l], par[z], l == 0 ? DenseSrc{x[z], net.L[0].Kp} : DenseSrc{(*acts[z])[l - 1], net.L[l - 1].Np}, (*acts[z])[l], bs);
        out.push_back(e);
    }
}
// mlp_backward_step of the nz instances of network `id` (the kind's network id: the index of o.dw, o.dw_grid and o.ra): the dX entries
// from the last layer down, the grouped dW, the reduce segments
template <class MemberArgs>
void dg_step_entries(MemberArgs& o, int id, const MlpLayout& net, int nz, float* const* p, float* const* g, float* const* m, float* const* v, float* const* tgt,
                     const float* x0, std::vector<float*>* const* acts, std::vector<float*>* const* dys, float* part, size_t part_stride,
                     const std::vector<size_t>& off, int bs, size_t total, double tau, const DenseReduceSeg* extra)
{
    const int L = (int)net.L.size();
    for (int l = L - 1; l >= 1; --l) {
        DenseGroupEntry e{};
        for (int z = 0; z < nz; ++z) e.a[z] = dg_dx_args(net.L[l], p[z], (*dys[z])[l], (*dys[z])[l - 1], (*acts[z])[l - 1], bs);
        o.dense.push_back(e);
    }
    DenseDwJob jobs[DW_GROUP];
    const int c = DenseAgent::chunks_for(bs);
    int nj = 0;
    for (int z = 0; z < nz; ++z)
        for (int l = 0; l < L; ++l)
            jobs[nj++] = DenseDwJob{&net.L[l], l == 0 ? DenseSrc{x0, net.L[0].Kp} : DenseSrc{(*acts[z])[l - 1], net.L[l - 1].Np}, (*dys[z])[l],
                                    part + (size_t)z * part_stride + off[l], c};
    o.dw_grid[id] = dense_dw_small_group_fill(o.dw[id], jobs, nj, bs);
    ReduceAdamArgs& ra = o.ra[id];
    ra = ReduceAdamArgs{};
    ra.nseg = L; ra.inst_part_stride = part_stride;
    for (int l = 0; l < L; ++l) {
        const DenseLayer& ly = net.L[l];
        const size_t nfl = (size_t)ly.Kp * ly.Np + ly.Np;
        ra.seg[l] = DenseReduceSeg{part + off[l], nfl, c, (unsigned)(ly.w / 4), (unsigned)(nfl / 4)};
    }
    if (extra) ra.seg[ra.nseg++] = *extra;
    for (int z = 0; z < nz; ++z) { ra.p[z] = p[z]; ra.g[z] = g[z]; ra.m[z] = m[z]; ra.v[z] = v[z]; ra.tgt[z] = tgt ? tgt[z] : nullptr; ra.vmax[z] = nullptr; }
    // (s[z], track and grads_only are the entry's: this step's words of the member's slot, the network, 0)
    ra.n4 = (unsigned)(total / 4); ra.track = tgt ? 1 : 0; ra.tau = (float)tau; ra.omt = (float)(1.0 - tau);
}

}  // namespace
