// ================================================================================================
// The group entries of dense.hpp's generic kernels with the member as grid dimension y and the network instance as grid dimension z,
// for launch groupings whose launches have instances (iql_group.hpp: IQL; awac_group.hpp: AWAC; candle_sac_group.hpp: candle SAC; the
// end-of-round ticket the groupings share is group_done.hpp), and the host half of a round that those kinds share.
// Each entry runs the body of the kernel it groups on the member's entry of a device array, read in place through the constant address
// space: member and instance come from blockIdx, so they are uniform and the entry's fields are scalar loads, as they are from the
// kernel-argument segment of the standalone kernel.  Same bodies, same bits.  (BC's own entries, with one instance, stay in bc_group.hpp,
// which does not include this header.)
// Bounds, for every kind on this header: member = blockIdx.y < gridDim.y = P = the length of gather and of every per-member array of
// the kind and of a step slot; z = blockIdx.z < gridDim.z = nz <= GP_MAXZ = the instances of a DenseGroupEntry and of a ReduceAdamArgs
// (2 n_critics <= GP_MAXZ is a condition of every group); the i-th forward / dX launch of the round (stream order) is handed
// dense + i * P and reads entry i * P + member, i < ndense = the kind's *_dense_launches: the array holds ndense * P entries; the
// weight-gradient and reduce + Adam launches of network n < NNET are handed dw + n * P / ra + n * P: NNET * P entries each, and
// NET < NNET <= the AdamScalars of the kind's Step.  Inside an instance every index is the body's own, with the bounds of the
// standalone kernel.  The reduce + Adam launch of a round that reads the step slot LAST ends with the ticket and publishes the round's
// launch number (bg_group_done - all workgroups of its three-dimensional grid counted, behind a barrier every thread reaches:
// dense_reduce_adam_body returns early for threads past the arena, to the entry, not out of the kernel).
// The host half below is what the kinds' rounds share: the writers of one member's entries - what mlp_forward / mlp_backward_step
// (dense_agent.hpp) hand the standalone launches of a network - into DenseMemberArgs, the staged arrays of the shared launches
// (DenseRound), and the walk over a round's plan (dg_round_launch), which launches gather, forward, dX, dW and reduce + Adam itself and
// hands the kind its own launches.
#pragma once
#include "dense.hpp"
#include "dense_agent.hpp"
#include "device_arrays.hpp"
#include "group_done.hpp"
#include "group_plan_common.hpp"

namespace {

static_assert(GP_DW_GROUP == DW_GROUP && GP_RA_SEGS == RA_SEGS && GP_MAXZ == RA_INST && GP_SHAPE_LAYERS >= BDR_MAX_UNITS + 1,
              "group_plan_common.hpp restates these limits");
// one member's arguments of one layer (or input-gradient) launch: instance z = blockIdx.z, as DenseArgsZ::a of the standalone launch
struct DenseGroupEntry { DenseArgs a[GP_MAXZ]; };

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
// The body of a kind's reduce + Adam entry, written once over the kind's per-step words: network NET of every member, instance
// z = blockIdx.z, the optimizer scalars from adam[NET] of the member's slot.  TRACK: the network tracks its targets at the member's own
// tau (a.tau / a.omt of its entry).  LAST: its launch is the last reader of the slot and publishes.
template <int NET, bool TRACK, bool LAST, class Step>
__device__ __forceinline__ void dg_reduce_adam_step(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS Step* steps, unsigned* ticket, unsigned* seq_host,
                                                    unsigned seq)
{
    const AdamScalars d = dg_step_scalars(steps[blockIdx.y].adam[NET]);
    dense_reduce_adam_body(args[blockIdx.y], (int)blockIdx.z, d, TRACK ? 1 : 0, 0);
    if constexpr (LAST) bg_group_done(ticket, seq_host, seq);
}
// a kind's table of its reduce + Adam entry's instantiations, indexed by network
template <class Step>
using DgReduceEntry = void (*)(const BDR_CONST_AS ReduceAdamArgs*, const BDR_CONST_AS Step*, unsigned*, unsigned*, unsigned);

// ---- host: one member's entries of the launches of one network (iql_group.hpp, awac_group.hpp, candle_sac_group.hpp) --------------------
// what every kind's MemberArgs holds: the gather, the forward and dX launches in stream order, and the weight-gradient and reduce
// entries by the kind's network id
template <int NNET>
struct DenseMemberArgs {
    GatherArgs gather;
    std::vector<DenseGroupEntry> dense;
    DenseDwSmallGroup dw[NNET]; int dw_grid[NNET];
    ReduceAdamArgs ra[NNET];
};
// the gather: k_gather's arguments as replay_sample_on_stream sets them (word_pos and size are this step's, read from the slot)
// (r: the member's ring or view; plan: replay_sample_plan's descriptor of this step)
inline GatherArgs dg_gather_static(const bdr_replay* r, const GatherArgs& plan)
{
    GatherArgs g = plan;
    replay_gather_shape(r->obs_bytes, &g.chunks, &g.vec_per_chunk);
    g.word_pos = 0; g.size = 0;
    return g;
}
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
template <int NNET>
void dg_step_entries(DenseMemberArgs<NNET>& o, int id, const MlpLayout& net, int nz, float* const* p, float* const* g, float* const* m, float* const* v, float* const* tgt,
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


// ---- host: the staged arrays of the shared launches and the walk over a round's plan ---------------------------------------------------
// The base of a kind (the K of group_core.hpp's GroupCore<K>) with NNET networks, whose plan numbers the weight gradient KDW and
// reduce + Adam KRA.  The kind adds the arrays of its own launches, its allocate / stage / upload over both, launch_own, and RA: its
// reduce + Adam entries by network.
template <int NNET, int KDW, int KRA>
struct DenseRound {
    static constexpr int NETS = NNET, K_DW = KDW, K_REDUCE_ADAM = KRA;
    int ndense = 0;   // forward and dX launches of a round
    StagedArray<GatherArgs> gather;                                            // [P]
    StagedArray<DenseGroupEntry> dense;                                        // [ndense][P] (launch order)
    StagedArray<DenseDwSmallGroup> dw; StagedArray<ReduceAdamArgs> ra;    // [NNET][P] by the kind's network id
    // In the order every kind has had: gather, pack, dense, the kind's own arrays (`own()`: its losses, then its samples), dW, reduce -
    // where the arrays lie in device memory shows in the round time (LAB.md, "One group core for the BC and the IQL group").
    template <class Pack, class Own>
    hipError_t allocate_round(int n_dense, size_t P, Pack& pack, Own own)
    {
        ndense = n_dense;
        hipError_t e = staged_resize(P, gather, pack);
        if (e == hipSuccess) e = dense.resize((size_t)ndense * P);
        if (e == hipSuccess) e = own();
        return e == hipSuccess ? staged_resize(NNET * P, dw, ra) : e;
    }
    // member p's entries of the shared launches into the staging arrays
    void stage_dense(size_t p, size_t P, const DenseMemberArgs<NNET>& o)
    {
        gather[p] = o.gather;
        for (int i = 0; i < ndense; ++i) dense[(size_t)i * P + p] = o.dense[i];
        for (int n = 0; n < NNET; ++n) { dw[(size_t)n * P + p] = o.dw[n]; ra[(size_t)n * P + p] = o.ra[n]; }
    }
    // the plan's dense launches and weight-gradient grids against the member's
    int32_t check_static(const GpLaunch* plan, int n_launches, const DenseMemberArgs<NNET>& o, uint32_t p) const
    {
        BDR_REQUIRE((int)o.dense.size() == ndense, "member %u: %d dense launches, the plan has %d", p, (int)o.dense.size(), ndense);
        for (int n = 0; n < n_launches; ++n)
            if (plan[n].kernel == KDW) {
                const int id = plan[n].net;
                BDR_REQUIRE(o.dw_grid[id] == (int)plan[n].gx, "member %u: the weight-gradient grid of network %d (%d) differs from the plan's (%u)", p, id, o.dw_grid[id],
                            plan[n].gx);
            }
        return BDR_OK;
    }
};

// One round's launches on the group's stream, grids from the plan; the kind's last reduce + Adam publishes `seq_no`.  The shared
// launches go out from here; every other one is the kind's: k.launch_own(l, n, P, grid, block, st, stream), which refuses a kernel id
// it does not know.
template <class G, class K>
int32_t dg_round_launch(const G& g, size_t P, const typename K::Step* steps_dev, unsigned seq_no, const K& k)
{
    using Step = typename K::Step;
    static_assert(sizeof(K::RA) / sizeof(K::RA[0]) == K::NETS, "one reduce + Adam entry per network");
    int nd = 0;
    hipStream_t stream = g.stream;
    const auto* st = (const BDR_CONST_AS Step*)steps_dev;
    for (int n = 0; n < g.n_launches; ++n) {
        const GpLaunch& l = g.plan[n];
        const dim3 grid(l.gx, l.gy, l.gz), block(l.threads);
        switch (l.kernel) {
        case GP_K_GATHER:
            BDR_TRY(replay_gather_group(stream, k.gather.d.get(), steps_dev, (uint32_t)sizeof(Step), (uint32_t)P, (uint64_t)g.shape.batch, (uint64_t)g.shape.obs_dim * 4));
            break;
        case GP_K_FWD:
        case GP_K_DX: {
            BDR_REQUIRE(nd < k.ndense, "%s group round: more dense launches in the plan than argument entries", K::NAME);
            const auto* a = (const BDR_CONST_AS DenseGroupEntry*)(k.dense.d.get() + (size_t)nd++ * P);
            if (l.kernel == GP_K_FWD) hipLaunchKernelGGL(k_dense_small_members_z<false>, grid, block, 0, stream, a);
            else hipLaunchKernelGGL(k_dense_small_members_z<true>, grid, block, 0, stream, a);
            break;
        }
        case K::K_DW:
            BDR_REQUIRE(l.net >= 0 && l.net < K::NETS, "%s group round: launch %d of the plan names no network", K::NAME, n);
            hipLaunchKernelGGL(k_dense_dw_small_members, grid, block, 0, stream, (const BDR_CONST_AS DenseDwSmallGroup*)(k.dw.d.get() + (size_t)l.net * P));
            break;
        case K::K_REDUCE_ADAM:
            BDR_REQUIRE(l.net >= 0 && l.net < K::NETS, "%s group round: launch %d of the plan names no network", K::NAME, n);
            hipLaunchKernelGGL(K::RA[l.net], grid, block, 0, stream, (const BDR_CONST_AS ReduceAdamArgs*)(k.ra.d.get() + (size_t)l.net * P), st, g.ticket.get(),
                               g.seq.dev, seq_no);
            break;
        default: BDR_TRY(k.launch_own(l, n, P, grid, block, st, stream));
        }
        BDR_HIP(hipGetLastError());
    }
    return BDR_OK;
}

}  // namespace
