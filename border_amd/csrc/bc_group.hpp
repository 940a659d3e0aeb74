// ================================================================================================
// A group of BC agents: Agent::opt of every member in the launch sequence Bc::opt enqueues for ONE member - gather, pack, the forward
// layers, the loss or the MFMA head, the input gradients, the grouped weight gradient, reduce + Adam - with every launch serving ALL
// members: the member index is grid dimension y (bc_group_plan.hpp has the rule and the grids).  A launch grouping, not an agent
// kind: the members stay ordinary BC agents on the group's stream.  A part of bc.hip's translation unit (it needs Bc and the bodies
// of BC's kernels), included where the code stands.
// Each entry below runs the body of the kernel it groups (bc.hip, dense.hpp, replay.hip) on args[member], read in place from a device
// array through the constant address space: the member index comes from blockIdx, so it is uniform and the member's fields are scalar
// loads, as they are from the kernel-argument segment of the existing entry.  Same bodies, same bits.  The loss and the head count
// gridDim.x workgroups on the member's OWN ticket: x stays the member's own grid.
// The host half - the members' adoption, the static argument arrays and their keys, the step ring and its slot rule, the round, records,
// sync - is group_core.hpp's, shared with the IQL group; BcGroupKind below says what is BC's.  Per step a member has a BcStep: the
// gather reads word_pos and size (GatherStepWords at its start), reduce + Adam its AdamScalars.  Reduce + Adam is the LAST launch of a
// round that reads the slot, so it ends with the ticket and publishes the round's launch number (bg_group_done - all workgroups of its
// two-dimensional grid counted, behind a barrier every thread reaches: dense_reduce_adam_body returns early for threads past the arena,
// to the entry, not out of the kernel).
// Bounds of every new index: member = blockIdx.y < P = the length of every argument array and of a slot; forward launch i reads
// d_dense[i * P + member], i < nfwd; input-gradient launch j reads d_dense[(nfwd + j) * P + member], j < ndx; the array holds
// (nfwd + ndx) * P entries.  Inside a member every index is the body's own, with the bounds of the standalone kernel.
#pragma once
#include "group_core.hpp"
#include "bc_group_plan.hpp"

static_assert(BG_FORM_DEFAULT == BDR_BC_KERNEL_DEFAULT && BG_FORM_GENERAL == BDR_BC_KERNEL_GENERAL && BG_FORM_FUSED == BDR_BC_KERNEL_FUSED &&
              BG_FORM_FUSED_MFMA == BDR_BC_KERNEL_FUSED_MFMA && BG_ACTION_DISCRETE == BDR_BC_ACTION_DISCRETE && BG_ACTION_CONTINUOUS == BDR_BC_ACTION_CONTINUOUS,
              "bc_group_plan.hpp restates these constants of border_amd.h");
static_assert(BG_DW_GROUP == DW_GROUP && BG_RA_SEGS == RA_SEGS && BG_SHAPE_LAYERS >= BDR_MAX_UNITS + 1, "bc_group_plan.hpp restates these limits");

// the per-step words of one member
struct BcStep { unsigned long long word_pos, size; AdamScalars adam; };
static_assert(offsetof(BcStep, word_pos) == offsetof(GatherStepWords, word_pos) && offsetof(BcStep, size) == offsetof(GatherStepWords, size),
              "the grouped gather reads the first two words of a member's BcStep");

namespace {

// (bg_group_done - gl_group_done's rule, group_layers.hpp: every workgroup of the launch counts, behind a barrier every thread reaches -
// lives in group_done.hpp, which the IQL group shares)

// ---- the group entries: grid dimension y is the member -------------------------------------------------------------------------------
__global__ void k_pack_rows_group(const BDR_CONST_AS PackRowsArgs* args)
{
    const BDR_CONST_AS PackRowsArgs& a = args[blockIdx.y];
    pack_rows_body(a.src, a.src_ld, a.cols, a.dst, a.ld, a.col0, a.B);
}
// a layer (DX = false) or an input gradient (DX = true)
template <bool DX>
__global__ __launch_bounds__(256) void k_bc_dense_small_group(const BDR_CONST_AS DenseArgs* args)
{
    __shared__ float red[4][32][33];
    dense_small_body<DX>(args[blockIdx.y], red);
}
__global__ __launch_bounds__(256) void k_bc_loss_group(const BDR_CONST_AS BcLossArgs* args) { bc_loss_body(args[blockIdx.y]); }
template <int NT>
__global__ __launch_bounds__(256) void k_bc_head_mfma_group(const BDR_CONST_AS BcHeadArgs* args) { bc_head_mfma_body<NT>(args[blockIdx.y]); }
__global__ __launch_bounds__(256) void k_bc_dense_dw_small_group(const BDR_CONST_AS DenseDwSmallGroup* args) { dense_dw_small_group_body(args[blockIdx.y]); }
// the member's optimizer scalars of this step come from its staging slot (track = 0, grads_only = 0); the last reader of the slot
__global__ __launch_bounds__(256) void k_bc_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS BcStep* steps, unsigned* ticket,
                                                              unsigned* seq_host, unsigned seq)
{
    const BDR_CONST_AS AdamScalars& s = steps[blockIdx.y].adam;
    AdamScalars d;   // field by field: static indices, registers
    d.b1 = s.b1; d.omb1 = s.omb1; d.b2 = s.b2; d.omb2 = s.omb2; d.sqrt_bc2 = s.sqrt_bc2; d.eps = s.eps; d.neg_step = s.neg_step; d.wd_mul = s.wd_mul;
    dense_reduce_adam_body(args[blockIdx.y], 0, d, 0, 0);
    bg_group_done(ticket, seq_host, seq);
}

// ---- group acting: Policy::sample of the selected members in ONE launch ----------------------------------------------------------------
// k_dense_act (dense_act.hpp) runs a whole acting call for a block of 32 rows in one workgroup on one CU, with no flags and no tickets
// between workgroups: for one agent one CU's matrix pipes bound it, for a group P members with a row each are P workgroups on P CUs.
// Grid x = the row blocks of ONE member's call (every selected member has the same n), grid y = the selected members.  The entry runs
// dense_act_body on args[member] (the network and the epilogue: static, in the group's device array) and calls[member] (the words of
// this call, in pinned, device-mapped memory), both read in place through the constant address space: member = sel[blockIdx.y] is
// uniform, so the member's fields stay scalar loads.  Same body, same tile order, same bits as the member's own k_dense_act, which
// tests/test_gpu_dense_act.py holds bit-equal to the layer path.  An acting call is synchronous: the launch ends with the ticket and
// publishes its launch number (bg_group_done) behind a system-scope fence of every thread's result stores, and the host waits for
// that number before it reads the results.
//   Bounds.  y < gridDim.y = the number of selected members = the length of `sel`; sel[y] < P = the length of `args` and `calls`
//   (checked by the host before anything is enqueued).  Inside a member every index is the body's own, with the standalone kernel's
//   bounds: rows are read for m0 + r < n and c < O from the member's staged block of n * O elements, out is written at
//   (m0 + r) * A + j < n * A inside the member's block of n * A floats.
// (the host half of an acting call - the member list, the checks, the staging areas, the launch number, the copy out - is
// group_act.hpp's, shared with the IQL group)
struct BcActCall { const uint8_t* rows; unsigned long long row_stride; const float* mean; const float* std; float* out; long long* idx; int n, f64; };

template <int TEAMS>
__global__ __launch_bounds__(256 * TEAMS) void k_bc_act_group(const BDR_CONST_AS DenseActArgs* args, const BDR_CONST_AS BcActCall* calls, const BDR_CONST_AS unsigned* sel,
                                                              unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    extern __shared__ __attribute__((aligned(16))) float da_lds[];
    const unsigned member = sel[blockIdx.y];
    dense_act_body<TEAMS, DA_EPI_BC>(args[member], calls[member], da_lds);
    __threadfence_system();   // this thread's result rows are in host memory before its workgroup counts
    bg_group_done(ticket, seq_host, seq);
}

BgShape bc_shape(const Bc* m)
{
    BgShape s{};
    s.obs_dim = m->O; s.act_dim = m->A; s.n_layers = (int)m->net.L.size();
    for (int i = 0; i < s.n_layers && i < BG_SHAPE_LAYERS; ++i) { s.Kp[i] = m->net.L[i].Kp; s.Np[i] = m->net.L[i].Np; s.out[i] = m->net.L[i].out; }
    s.batch = (int)m->cfg.batch_size; s.activation_out = m->cfg.policy.activation_out; s.form = m->form; s.action_type = m->cfg.action_type;
    return s;
}

// ---- host: one member's static arguments, exactly what Bc::update hands its launches ---------------------------------------------------
struct BcMemberArgs {
    GatherArgs gather; PackRowsArgs pack;
    DenseArgs fwd[BG_SHAPE_LAYERS]; DenseArgs dx[BG_SHAPE_LAYERS];   // fwd[i]: layer i; dx[i]: the gradient w.r.t. layer i's input (i >= 1)
    BcLossArgs loss; BcHeadArgs head;
    DenseDwSmallGroup dw; int dw_grid;
    ReduceAdamArgs ra;
};

// (bs: the batch size; r: the member's ring or view; plan: replay_sample_plan's descriptor of this step)
void bc_member_static(Bc* m, int bs, const bdr_replay* r, const GatherArgs& plan, BcMemberArgs& o)
{
    memset(&o, 0, sizeof o);
    const MlpLayout& net = m->net;
    const int L = (int)net.L.size();
    const bool head = m->form == BDR_BC_KERNEL_FUSED_MFMA;
    const DenseLayer& last = net.L[L - 1];
    const float* data = reinterpret_cast<const float*>(r->b_act);
    const float inv_n = (float)(1.0 / ((double)bs * (double)m->A));
    // the gather: k_gather's arguments as replay_sample_on_stream sets them (word_pos and size are this step's, read from the slot)
    o.gather = plan;
    replay_gather_shape(r->obs_bytes, &o.gather.chunks, &o.gather.vec_per_chunk);
    o.gather.word_pos = 0; o.gather.size = 0;
    o.pack = PackRowsArgs{reinterpret_cast<const float*>(r->b_obs), m->O, m->O, m->x0, net.L[0].Kp, 0, bs};
    // mlp_forward / dense_forward_z of every layer the head does not take
    DenseSrc in{m->x0, net.L[0].Kp};
    for (int i = 0; i < (head ? L - 1 : L); ++i) {
        const DenseLayer& l = net.L[i];
        DenseArgs& d = o.fwd[i];
        d.x = in; d.w = m->p + l.w; d.bias = m->p + l.b; d.out = m->act[i]; d.ldo = l.Np;
        d.M = bs; d.ncols = l.Np; d.kred = l.Kp; d.relu = l.relu; d.w_ld = l.Np;
        in = DenseSrc{m->act[i], l.Np};
    }
    if (head)
        o.head = BcHeadArgs{m->act[L - 2], last.Kp, m->p + last.w, m->p + last.b, data, m->A, bs, m->cfg.policy.activation_out,
                            m->pred, m->dy[L - 1], m->dy[L - 2], m->rowsq, m->ticket, m->scal, 0, inv_n};
    else
        o.loss = BcLossArgs{m->act[L - 1], last.Np, data, m->A, bs, m->cfg.policy.activation_out, m->pred, m->dy[L - 1], m->rowsq, m->ticket, m->scal, 0, inv_n};
    // mlp_backward_step: dense_dx_z down the net
    for (int i = head ? L - 2 : L - 1; i > 0; --i) {
        const DenseLayer& l = net.L[i];
        DenseArgs& d = o.dx[i];
        d.x = DenseSrc{m->dy[i], l.Np}; d.w = m->p + l.w; d.out = m->dy[i - 1]; d.ldo = l.Kp; d.mask = m->act[i - 1]; d.ldm = l.Kp;
        d.M = bs; d.ncols = l.Kp; d.kred = l.Np; d.w_ld = l.Np;
    }
    // the grouped weight gradient and the reduce segments over the member's own partials
    DenseDwJob jobs[DW_GROUP];
    const int c = DenseAgent::chunks_for(bs);
    for (int i = 0; i < L; ++i)
        jobs[i] = DenseDwJob{&net.L[i], i == 0 ? DenseSrc{m->x0, net.L[0].Kp} : DenseSrc{m->act[i - 1], net.L[i - 1].Np}, m->dy[i], m->part + m->off[i], c};
    o.dw_grid = dense_dw_small_group_fill(o.dw, jobs, L, bs);
    ReduceAdamArgs& ra = o.ra;
    ra.nseg = L;
    for (int i = 0; i < L; ++i) {
        const size_t nfl = (size_t)net.L[i].Kp * net.L[i].Np + net.L[i].Np;
        ra.seg[i] = DenseReduceSeg{m->part + m->off[i], nfl, c, (unsigned)(net.L[i].w / 4), (unsigned)(nfl / 4)};
    }
    ra.p[0] = m->p; ra.g[0] = m->g; ra.m[0] = m->m; ra.v[0] = m->v; ra.n4 = (unsigned)(net.total / 4);
    ra.tau = 0.f; ra.omt = 1.f;   // (no target: track == 0; s[0] is this step's: BcStep)
}

// ---- what is BC's of the group core (group_core.hpp) -------------------------------------------------------------------------------------
// group acting: the policy net on the member's arena, bc_act_out of its activation_out, no words beyond the common ones
struct BcActKind : GroupActEntry<BcActCall, k_bc_act_group<1>, k_bc_act_group<2>> {
    const float* arena(const Bc* m) const { return m->p; }
    void write_static(const Bc* m, DenseActArgs& a) const
    {
        a.nl = (int)m->net.L.size();
        for (int l = 0; l < a.nl; ++l) a.L[l] = DenseActLayer{m->p + m->net.L[l].w, m->p + m->net.L[l].b, m->net.L[l].Kp, m->net.L[l].Np, m->net.L[l].relu};
        a.mode = DA_BC; a.kind = m->cfg.policy.activation_out;
    }
    void noise(const Bc*, int*, uint64_t*) const {}   // (no noise stream: nothing draws)
    void call_words(Bc*, BcActCall&, int, uint64_t, uint64_t) const {}
};

struct BcGroupKind {
    using Member = Bc; using Shape = BgShape; using Launch = BgLaunch; using Step = BcStep; using MemberArgs = BcMemberArgs; using PlanMember = BgMember;
    using Act = BcActKind;
    static constexpr const char *KIND = "bc", *A = "a BC", *NAME = "BC", *CAP_MSG = "cap_per_member must be positive";
    static constexpr int MAX_LAUNCHES = BG_MAX_LAUNCHES, K_GATHER = BG_K_GATHER, FORM = BDR_GROUP_FORM_BC_LAYERS, MIN_CAP = 1;
    static BgMember describe(const Bc* m) { return BgMember{bc_shape(m), m->device, m->prof ? 1 : 0, m->grad_comm ? 1 : 0, m}; }
    static int refusal(const BgMember* m, unsigned n, const char** why, int* kernel) { return bg_group_refusal(m, n, why, kernel); }
    static const char* kernel_name(int k) { return bg_kernel_name(k); }
    static int round_plan(const BgShape& s, unsigned P, BgLaunch* out) { return bg_round_plan(s, P, out); }
    static int launch_count(const BgShape& s) { return bg_launch_count(s.n_layers, s.form); }
    // Bc::opt / Bc::update on the host
    static BcStep fill_step(Bc* m, int bs, const GatherArgs& plan)
    {
        m->step += 1;
        const AdamScalars sc = DenseAgent::opt_scalars(m->cfg.opt, m->cfg.lr, m->step);
        m->n_opts += 1;
        m->last_B = bs;
        return BcStep{plan.word_pos, plan.size, sc};
    }
    static void member_static(Bc* m, int bs, const bdr_replay* r, const GatherArgs& plan, BcMemberArgs& o) { bc_member_static(m, bs, r, plan, o); }

    int L = 0, nfwd = 0, ndx = 0, head = 0;
    StagedArray<GatherArgs> gather; StagedArray<PackRowsArgs> pack; StagedArray<BcLossArgs> loss; StagedArray<BcHeadArgs> hd;
    StagedArray<DenseDwSmallGroup> dw; StagedArray<ReduceAdamArgs> ra;
    StagedArray<DenseArgs> dense;   // [nfwd][P] then [ndx][P] (launch order)
    hipError_t allocate(const BgShape& s, size_t P)
    {
        L = s.n_layers;
        head = s.form == BG_FORM_FUSED_MFMA ? 1 : 0;
        nfwd = head ? L - 1 : L;
        ndx = head ? L - 2 : L - 1;
        hipError_t e = staged_resize(P, gather, pack);   // (in this order: where the arrays lie in device memory shows in the round time, LAB.md)
        if (e == hipSuccess) e = dense.resize((size_t)(nfwd + ndx) * P);
        return e == hipSuccess ? staged_resize(P, loss, hd, dw, ra) : e;
    }
    // member p's arguments into the staging arrays
    void stage(size_t p, size_t P, const BcMemberArgs& o)
    {
        gather[p] = o.gather; pack[p] = o.pack; loss[p] = o.loss; hd[p] = o.head; dw[p] = o.dw; ra[p] = o.ra;
        for (int i = 0; i < nfwd; ++i) dense[(size_t)i * P + p] = o.fwd[i];
        for (int j = 0; j < ndx; ++j) dense[(size_t)(nfwd + j) * P + p] = o.dx[(head ? L - 2 : L - 1) - j];   // j-th dX launch of the round
    }
    hipError_t upload() { return staged_upload(gather, pack, dense, loss, hd, dw, ra); }
    int32_t check_static(const BgLaunch* plan, int n, const BcMemberArgs& o, uint32_t p) const
    {
        BDR_REQUIRE(o.dw_grid == (int)plan[n - 2].gx, "member %u: the weight-gradient grid (%d) differs from the plan's (%u)", p, o.dw_grid, plan[n - 2].gx);
        return BDR_OK;
    }
    // one round's launches on the group's stream, grids from the plan; the last one publishes `seq_no`
    int32_t launch(const GroupCore<BcGroupKind>& g, size_t P, const BcStep* steps_dev, unsigned seq_no) const
    {
        int fwd = 0, dx = 0;
        for (int n = 0; n < g.n_launches; ++n) {
            const BgLaunch& l = g.plan[n];
            const dim3 grid(l.gx, l.gy, l.gz), block(l.threads);
            switch (l.kernel) {
            case BG_K_GATHER:
                BDR_TRY(replay_gather_group(g.stream, gather.d.get(), steps_dev, (uint32_t)sizeof(BcStep), (uint32_t)P, (uint64_t)g.shape.batch, (uint64_t)g.shape.obs_dim * 4));
                break;
            case BG_K_PACK: hipLaunchKernelGGL(k_pack_rows_group, grid, block, 0, g.stream, (const BDR_CONST_AS PackRowsArgs*)pack.d.get()); break;
            case BG_K_FWD:
                hipLaunchKernelGGL(k_bc_dense_small_group<false>, grid, block, 0, g.stream, (const BDR_CONST_AS DenseArgs*)(dense.d.get() + (size_t)fwd++ * P));
                break;
            case BG_K_LOSS: hipLaunchKernelGGL(k_bc_loss_group, grid, block, 0, g.stream, (const BDR_CONST_AS BcLossArgs*)loss.d.get()); break;
            case BG_K_HEAD:
                if (g.shape.act_dim <= 32) hipLaunchKernelGGL(k_bc_head_mfma_group<1>, grid, block, 0, g.stream, (const BDR_CONST_AS BcHeadArgs*)hd.d.get());
                else hipLaunchKernelGGL(k_bc_head_mfma_group<2>, grid, block, 0, g.stream, (const BDR_CONST_AS BcHeadArgs*)hd.d.get());
                break;
            case BG_K_DX:
                hipLaunchKernelGGL(k_bc_dense_small_group<true>, grid, block, 0, g.stream, (const BDR_CONST_AS DenseArgs*)(dense.d.get() + (size_t)(nfwd + dx++) * P));
                break;
            case BG_K_DW: hipLaunchKernelGGL(k_bc_dense_dw_small_group, grid, block, 0, g.stream, (const BDR_CONST_AS DenseDwSmallGroup*)dw.d.get()); break;
            case BG_K_REDUCE_ADAM:
                hipLaunchKernelGGL(k_bc_reduce_adam_group, grid, block, 0, g.stream, (const BDR_CONST_AS ReduceAdamArgs*)ra.d.get(), (const BDR_CONST_AS BcStep*)steps_dev,
                                   g.ticket.get(), g.seq.dev, seq_no);
                break;
            default: return fail(BDR_ERR_INVALID, "BC group round: launch %d of the plan names no kernel", n);
            }
            BDR_HIP(hipGetLastError());
        }
        return BDR_OK;
    }
};

}  // namespace

struct bdr_bc_group : GroupCore<BcGroupKind> {};

namespace bdr {
int bc_group_act_dim(const void* group, uint32_t member) { return group_act_dim<bdr_bc_group>(group, member); }   // (trainer.hip)
}  // namespace bdr

extern "C" {

int32_t bdr_bc_group_create(bdr_agent* const* agents, uint32_t n, bdr_bc_group** out) { return group_create(agents, n, out); }
int32_t bdr_bc_group_destroy(bdr_bc_group* g) { return group_destroy(g); }
int32_t bdr_bc_group_size(const bdr_bc_group* g, uint32_t* n) { return group_size(g, n); }
int32_t bdr_bc_group_member(const bdr_bc_group* g, uint32_t i, bdr_agent** out) { return group_member(g, i, out); }
int32_t bdr_bc_group_info(const bdr_bc_group* g, bdr_group_info* out) { return group_info(g, out); }
int32_t bdr_bc_group_opt(bdr_bc_group* g, bdr_replay* const* buffers) { return group_opt(g, buffers); }
int32_t bdr_bc_group_opt_with_scalars(bdr_bc_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    return group_opt_with_scalars(g, buffers, out, cap_per_member, n_out);
}
int32_t bdr_bc_group_sample(bdr_bc_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    return group_sample(g, norms, n, rows, dtypes, act_out);
}
int32_t bdr_bc_group_sample_members(bdr_bc_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n,
                                    const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    return group_sample_members(g, members, n_sel, norms, n, rows, dtypes, act_out);
}
int32_t bdr_bc_group_sync(bdr_bc_group* g) { return group_sync(g); }
int32_t bdr_bc_group_copy_members(bdr_bc_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags)
{
    return group_copy_members(g, src, dst, n, flags);
}

}  // extern "C"
