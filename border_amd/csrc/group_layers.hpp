// ================================================================================================
// The layer form of an agent group: members that do not take the one-workgroup step (Mlp[256, 256] at batch 64, the reference's own
// CartPole example, and every net between it and Mlp[64, 64]) stepped by the launch sequence DqnMlp::update_critic enqueues for ONE
// such member on its latency-shaped layer path - gather, pack, the forward layers, the row-block head (or TD rows + loss mean), the
// input gradients, the grouped weight gradient, reduce + Adam with the soft update riding on it - with every launch serving ALL
// members: the member index is one grid dimension (group_layers_plan.hpp has the rule and the grids).  A part of mlp_agents.hip's
// translation unit, included from agent_group.hpp.
// Each entry below runs the body of the kernel it groups (dense.hpp, mlp_agents.hip, replay.hip) on args[member], read in place
// from a device array through the constant address space: the member index comes from blockIdx, so it is uniform and the member's
// fields are scalar loads, as they are from the kernel-argument segment of the existing entry.  Same bodies, same bits.
//   static arguments   one device array per kernel family (GroupLayers), rewritten with bdr_agent_group::d_args' rule: only when a
//                      member's buffers or ring change, synchronously, behind a stream synchronise
//   per step           MfStep[P] in a slot of the group's step ring: the gather reads word_pos and size of the member's entry, reduce +
//                      Adam its AdamScalars, do_adam and do_track
// The slot rule: reduce + Adam is the LAST launch of a round that reads the slot, so it ends with the ticket and publishes the round's
// launch number (gl_group_done - all workgroups of its two-dimensional grid counted, behind a barrier every thread reaches: the body
// returns early for threads past the arena, to the entry, not out of the kernel).
#pragma once
#include "group_layers_plan.hpp"

static_assert(GL_MAXL == MF_MAXL && GL_RA_SEGS == RA_SEGS && GL_MAXL <= DW_GROUP, "group_layers_plan.hpp restates these limits");
static_assert(offsetof(MfStep, word_pos) == offsetof(GatherStepWords, word_pos) && offsetof(MfStep, size) == offsetof(GatherStepWords, size),
              "the grouped gather reads the first two words of a member's MfStep");

namespace {

// mf_group_done for a grid of any rank: every workgroup of the launch counts
__device__ __forceinline__ void gl_group_done(unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x * gridDim.y * gridDim.z - 1) {
        atomicExch(ticket, 0u);   // (the next launch is behind this one in the stream)
        __hip_atomic_store(seq_host, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- the group entries: grid dimension y is the member (z for the row-block head, whose body owns x and y) ----------------------
__global__ void k_mlp_pack_z_group(const BDR_CONST_AS MlpPackArgs* args) { mlp_pack_z_body(args[blockIdx.y]); }
// a layer (DX = false) or an input gradient (DX = true): args[member][zs] with instance z = blockIdx.z
template <bool DX>
__global__ __launch_bounds__(256) void k_dense_small_group(const BDR_CONST_AS DenseArgs* args, unsigned zs)
{
    __shared__ float red[4][32][33];
    dense_small_body<DX>(args[(size_t)blockIdx.y * zs + blockIdx.z], red);
}
__global__ __launch_bounds__(512) void k_mlp_head_td_group(const BDR_CONST_AS MlpHeadTdArgs* args) { mlp_head_td_body(args[blockIdx.z]); }
__global__ __launch_bounds__(256) void k_td_dense_group(const BDR_CONST_AS TdDenseArgs* args) { td_dense_body(args[blockIdx.y]); }
struct MeanRowsArgs { const float* x; int n; float* out; float scale; };
__global__ __launch_bounds__(256) void k_mean_rows_group(const BDR_CONST_AS MeanRowsArgs* args)
{
    const BDR_CONST_AS MeanRowsArgs& a = args[blockIdx.y];
    mean_rows_body(a.x, a.n, a.out, a.scale);
}
__global__ __launch_bounds__(256) void k_dense_dw_small_group_members(const BDR_CONST_AS DenseDwSmallGroup* args) { dense_dw_small_group_body(args[blockIdx.y]); }
__global__ __launch_bounds__(256) void k_dense_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS MfStep* steps, unsigned* ticket,
                                                                 unsigned* seq_host, unsigned seq)
{
    const MfStep d = mf_step_load(steps[blockIdx.y]);
    dense_reduce_adam_body(args[blockIdx.y], 0, d.adam, d.do_track, d.do_adam ? 0 : 1);
    gl_group_done(ticket, seq_host, seq);
}

// ---- host: one member's static arguments, exactly what DqnMlp::update_critic hands its launches -----------------------------------
struct GlMemberArgs {
    GatherArgs gather; MlpPackArgs pack;
    DenseArgs fwd[GL_MAXL][MAXZ]; DenseArgs dx[GL_MAXL];   // fwd[i]: layer i of every instance; dx[i]: the gradient w.r.t. layer i's input (i >= 1)
    MlpHeadTdArgs head; TdDenseArgs td; MeanRowsArgs mean;
    DenseDwSmallGroup dw; int dw_grid;
    ReduceAdamArgs ra;
};

// (bs: the batch size; r: the member's uniform ring; plan: replay_sample_plan's descriptor of this step)
void gl_member_static(DqnMlp* m, int bs, const bdr_replay* r, const GatherArgs& plan, GlMemberArgs& o)
{
    memset(&o, 0, sizeof o);
    const MlpLayout& net = m->net;
    const int L = (int)net.L.size(), nz = m->cfg.double_dqn ? 3 : 2;
    const bool head = gl_head_fused(m->gl_shape(bs));
    const float* par[MAXZ] = {m->q, m->q_tgt, m->q};
    // the gather: k_gather's arguments as replay_sample_on_stream sets them (word_pos and size are this step's, read from the slot)
    o.gather = plan;
    replay_gather_shape(r->obs_bytes, &o.gather.chunks, &o.gather.vec_per_chunk);
    o.gather.word_pos = 0; o.gather.size = 0;
    // k_mlp_pack_z
    o.pack.rows[0] = reinterpret_cast<const float*>(r->b_obs); o.pack.rows[1] = o.pack.rows[2] = reinterpret_cast<const float*>(r->b_next);
    for (int z = 0; z < nz; ++z) o.pack.x[z] = m->x_in[z];
    o.pack.nz = nz; o.pack.B = bs; o.pack.in_dim = net.in_dim; o.pack.Kp0 = net.L[0].Kp;
    // dense_forward_z of every layer the head does not take
    DenseSrc in[MAXZ];
    for (int z = 0; z < nz; ++z) in[z] = DenseSrc{m->x_in[z], net.L[0].Kp};
    for (int i = 0; i < (head ? L - 1 : L); ++i) {
        const DenseLayer& l = net.L[i];
        for (int z = 0; z < nz; ++z) {
            DenseArgs& d = o.fwd[i][z];
            d.x = in[z]; d.w = par[z] + l.w; d.bias = par[z] + l.b; d.out = m->acts[z][i]; d.ldo = l.Np;
            d.M = bs; d.ncols = l.Np; d.kred = l.Kp; d.relu = l.relu; d.w_ld = l.Np;
            in[z] = DenseSrc{m->acts[z][i], l.Np};
        }
    }
    // TdDenseArgs (uniform ring: no weights)
    TdDenseArgs& t = o.td;
    t.q_on = m->acts[0][L - 1]; t.q_tg = m->acts[1][L - 1]; t.q_on_next = m->cfg.double_dqn ? m->acts[2][L - 1] : nullptr;
    t.ld = net.L[L - 1].Np; t.act = r->b_act; t.act_bytes = (int)r->act_bytes; t.reward = r->b_reward; t.term = r->b_term;
    t.dq_rows = m->dys[L - 1]; t.pred = m->pred; t.tgt = m->tgt; t.loss_row = m->loss_row;
    t.B = bs; t.A = net.out_dim; t.gamma = (float)m->cfg.discount_factor; t.loss_kind = m->cfg.critic_loss;
    t.weight = nullptr; t.td_abs = m->td_abs;
    t.has_clip = m->cfg.has_clip_td_err; t.clip_min = (float)m->cfg.clip_td_err_min; t.clip_max = (float)m->cfg.clip_td_err_max;
    t.err = m->dev_err; t.relu_out = net.L[L - 1].relu;
    o.mean = MeanRowsArgs{m->loss_row, bs, m->loss, 1.0f / (float)bs};
    if (head) {
        const DenseLayer& ll = net.L[L - 1];
        MlpHeadTdArgs& h = o.head;
        h.nz = nz;
        for (int z = 0; z < nz; ++z) { h.hin[z] = m->acts[z][L - 2]; h.wl[z] = HeadRef{par[z] + ll.w, par[z] + ll.b, ll.relu}; h.q[z] = m->acts[z][L - 1]; }
        h.ldh = ll.Kp; h.kred = ll.Kp; h.w_ld = ll.Np; h.ldq = ll.Np; h.sel_z = m->cfg.double_dqn ? 2 : -1;
        h.t = t; h.w_last = m->q + ll.w; h.dh = m->dys[L - 2]; h.ticket = m->ticket; h.loss = m->loss; h.scale = 1.0f / (float)bs;
    }
    // dense_dx down the net
    for (int i = head ? L - 2 : L - 1; i > 0; --i) {
        const DenseLayer& l = net.L[i];
        DenseArgs& d = o.dx[i];
        d.accum = 0;
        d.x = DenseSrc{m->dys[i], l.Np}; d.w = m->q + l.w; d.out = m->dys[i - 1]; d.ldo = l.Kp; d.mask = m->acts[0][i - 1]; d.ldm = l.Kp;
        d.M = bs; d.ncols = l.Kp; d.kred = l.Np; d.w_ld = l.Np;
    }
    // the grouped weight gradient and the reduce segments over the member's own partials
    DenseDwJob jobs[RA_SEGS];
    for (int i = 0; i < L; ++i)
        jobs[i] = DenseDwJob{&net.L[i], i == 0 ? DenseSrc{m->x_in[0], net.L[0].Kp} : DenseSrc{m->acts[0][i - 1], net.L[i - 1].Np}, m->dys[i], m->dw_part + m->dw_off[i],
                             std::min(m->dw_chunks_l[i], std::max(1, bs / 256))};
    o.dw_grid = dense_dw_small_group_fill(o.dw, jobs, L, bs);
    ReduceAdamArgs& ra = o.ra;
    ra.nseg = L;
    for (int i = 0; i < L; ++i) {
        const size_t nfl = (size_t)net.L[i].Kp * net.L[i].Np + net.L[i].Np;
        ra.seg[i] = DenseReduceSeg{m->dw_part + m->dw_off[i], nfl, jobs[i].chunks, (unsigned)(net.L[i].w / 4), (unsigned)(nfl / 4)};
    }
    ra.p[0] = m->q; ra.g[0] = m->grad; ra.m[0] = m->m; ra.v[0] = m->v; ra.tgt[0] = m->q_tgt; ra.n4 = (unsigned)(net.total / 4);
    ra.tau = (float)m->cfg.tau; ra.omt = (float)(1.0 - m->cfg.tau);   // (s[0], track and grads_only are this step's: MfStep)
}

// the device arrays of a layer-form group and their host staging, one per kernel family
struct GroupLayers {
    GlShape shape{};                 // the one shape of all members
    GlLaunch plan[GL_MAX_LAUNCHES]; int n_launches = 0;
    int nfwd = 0, ndx = 0, head = 0;
    std::vector<GatherArgs> h_gather; DeviceArray<GatherArgs> d_gather;
    std::vector<MlpPackArgs> h_pack; DeviceArray<MlpPackArgs> d_pack;
    std::vector<DenseArgs> h_dense; DeviceArray<DenseArgs> d_dense;     // [nfwd][P][MAXZ] then [ndx][P] (launch order)
    std::vector<MlpHeadTdArgs> h_head; DeviceArray<MlpHeadTdArgs> d_head;
    std::vector<TdDenseArgs> h_td; DeviceArray<TdDenseArgs> d_td;
    std::vector<MeanRowsArgs> h_mean; DeviceArray<MeanRowsArgs> d_mean;
    std::vector<DenseDwSmallGroup> h_dw; DeviceArray<DenseDwSmallGroup> d_dw;
    std::vector<ReduceAdamArgs> h_ra; DeviceArray<ReduceAdamArgs> d_ra;
    size_t fwd_at(int i, size_t P) const { return (size_t)i * P * MAXZ; }
    size_t dx_at(int j, size_t P) const { return (size_t)nfwd * P * MAXZ + (size_t)j * P; }   // j-th dX launch of the round

    hipError_t allocate(const GlShape& s, size_t P)
    {
        shape = s;
        n_launches = gl_round_plan(s, (unsigned)P, plan);
        head = gl_head_fused(s) ? 1 : 0;
        nfwd = head ? s.n_layers - 1 : s.n_layers;
        ndx = (head ? s.n_layers - 2 : s.n_layers - 1);
        h_gather.resize(P); h_pack.resize(P); h_dense.resize((size_t)nfwd * P * MAXZ + (size_t)ndx * P); h_head.resize(P); h_td.resize(P); h_mean.resize(P);
        h_dw.resize(P); h_ra.resize(P);
        hipError_t e = device_array(d_gather, P);
        if (e == hipSuccess) e = device_array(d_pack, P);
        if (e == hipSuccess) e = device_array(d_dense, h_dense.size());
        if (e == hipSuccess) e = device_array(d_head, P);
        if (e == hipSuccess) e = device_array(d_td, P);
        if (e == hipSuccess) e = device_array(d_mean, P);
        if (e == hipSuccess) e = device_array(d_dw, P);
        if (e == hipSuccess) e = device_array(d_ra, P);
        return e;
    }
    // member p's arguments into the staging arrays
    void stage(size_t p, size_t P, const GlMemberArgs& o)
    {
        const int L = shape.n_layers;
        h_gather[p] = o.gather; h_pack[p] = o.pack; h_head[p] = o.head; h_td[p] = o.td; h_mean[p] = o.mean; h_dw[p] = o.dw; h_ra[p] = o.ra;
        for (int i = 0; i < nfwd; ++i) for (int z = 0; z < MAXZ; ++z) h_dense[fwd_at(i, P) + p * MAXZ + z] = o.fwd[i][z];
        for (int j = 0; j < ndx; ++j) h_dense[dx_at(j, P) + p] = o.dx[(head ? L - 2 : L - 1) - j];
    }
    hipError_t upload(size_t P)
    {
        hipError_t e = hipMemcpy(d_gather.get(), h_gather.data(), P * sizeof(GatherArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_pack.get(), h_pack.data(), P * sizeof(MlpPackArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_dense.get(), h_dense.data(), h_dense.size() * sizeof(DenseArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_head.get(), h_head.data(), P * sizeof(MlpHeadTdArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_td.get(), h_td.data(), P * sizeof(TdDenseArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_mean.get(), h_mean.data(), P * sizeof(MeanRowsArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_dw.get(), h_dw.data(), P * sizeof(DenseDwSmallGroup), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_ra.get(), h_ra.data(), P * sizeof(ReduceAdamArgs), hipMemcpyHostToDevice);
        return e;
    }
    // one round's launches on `stream`, grids from the plan; the last one publishes `seq`
    int32_t launch(hipStream_t stream, size_t P, const MfStep* steps_dev, unsigned* ticket, unsigned* seq_host, unsigned seq)
    {
        int fwd = 0, dx = 0;
        for (int n = 0; n < n_launches; ++n) {
            const GlLaunch& l = plan[n];
            const dim3 grid(l.gx, l.gy, l.gz), block(l.threads);
            switch (l.kernel) {
            case GL_K_GATHER:
                BDR_TRY(replay_gather_group(stream, d_gather.get(), steps_dev, (uint32_t)sizeof(MfStep), (uint32_t)P, (uint64_t)shape.batch, (uint64_t)shape.in_dim * 4));
                break;
            case GL_K_PACK: hipLaunchKernelGGL(k_mlp_pack_z_group, grid, block, 0, stream, (const BDR_CONST_AS MlpPackArgs*)d_pack.get()); break;
            case GL_K_FWD:
                hipLaunchKernelGGL(k_dense_small_group<false>, grid, block, 0, stream, (const BDR_CONST_AS DenseArgs*)(d_dense.get() + fwd_at(fwd++, P)), (unsigned)MAXZ);
                break;
            case GL_K_HEAD_TD: hipLaunchKernelGGL(k_mlp_head_td_group, grid, block, 0, stream, (const BDR_CONST_AS MlpHeadTdArgs*)d_head.get()); break;
            case GL_K_TD_DENSE: hipLaunchKernelGGL(k_td_dense_group, grid, block, 0, stream, (const BDR_CONST_AS TdDenseArgs*)d_td.get()); break;
            case GL_K_MEAN_ROWS: hipLaunchKernelGGL(k_mean_rows_group, grid, block, 0, stream, (const BDR_CONST_AS MeanRowsArgs*)d_mean.get()); break;
            case GL_K_DX:
                hipLaunchKernelGGL(k_dense_small_group<true>, grid, block, 0, stream, (const BDR_CONST_AS DenseArgs*)(d_dense.get() + dx_at(dx++, P)), 1u);
                break;
            case GL_K_DW: hipLaunchKernelGGL(k_dense_dw_small_group_members, grid, block, 0, stream, (const BDR_CONST_AS DenseDwSmallGroup*)d_dw.get()); break;
            case GL_K_REDUCE_ADAM:
                hipLaunchKernelGGL(k_dense_reduce_adam_group, grid, block, 0, stream, (const BDR_CONST_AS ReduceAdamArgs*)d_ra.get(), (const BDR_CONST_AS MfStep*)steps_dev,
                                   ticket, seq_host, seq);
                break;
            default: return fail(BDR_ERR_INVALID, "layer-form round: launch %d of the plan names no kernel", n);
            }
            BDR_HIP(hipGetLastError());
        }
        return BDR_OK;
    }
};

}  // namespace
