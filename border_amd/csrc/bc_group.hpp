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
//   static arguments   one device array per kernel family, rewritten only when a member's buffers or ring change (`keys`),
//                      synchronously, behind a stream synchronise: rare
//   per step           BcStep[P] in a slot of the pinned, device-mapped step ring: the gather reads word_pos and size of the member's
//                      entry (GatherStepWords at its start), reduce + Adam its AdamScalars
// The slot rule (slot_ring.hpp): reduce + Adam is the LAST launch of a round that reads the slot, so it ends with the ticket and
// publishes the round's launch number (bg_group_done - all workgroups of its two-dimensional grid counted, behind a barrier every
// thread reaches: dense_reduce_adam_body returns early for threads past the arena, to the entry, not out of the kernel).  The host
// rewrites a slot only once the pinned word has reached the number recorded for it: no copy command, event or synchronise in the
// steady loop.
// Bounds of every new index: member = blockIdx.y < P = the length of every argument array and of a slot; forward launch i reads
// d_dense[i * P + member], i < nfwd; input-gradient launch j reads d_dense[(nfwd + j) * P + member], j < ndx; the array holds
// (nfwd + ndx) * P entries.  Inside a member every index is the body's own, with the bounds of the standalone kernel.
#pragma once
#include "slot_ring.hpp"
#include "device_arrays.hpp"
#include "group_done.hpp"
#include "group_act.hpp"
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

}  // namespace

struct bdr_bc_group {
    enum { STEP_SLOTS = 8 };
    int32_t device = 0;
    hipStream_t stream = nullptr;
    // (bdr_bc_group_destroy has synchronised the stream and destroyed the members; a failed create has adopted nobody.)  The stream
    // goes first, the buffers - the members below - after it.
    ~bdr_bc_group() { if (stream) { stream_retire(stream); (void)hipStreamDestroy(stream); } }
    std::vector<Bc*> members;
    BgShape shape{};                 // the one shape of all members
    BgLaunch plan[BG_MAX_LAUNCHES]; int n_launches = 0;
    int nfwd = 0, ndx = 0, head = 0;
    uint64_t kernel_launches = 0;    // every kernel launch the group's own calls have enqueued (bdr_bc_group_info)
    struct StaticKey { bool valid = false; uint64_t batch_gen = 0, r_uid = 0, r_batch_gen = 0; };
    std::vector<StaticKey> keys;
    std::vector<GatherArgs> h_gather; DeviceArray<GatherArgs> d_gather;
    std::vector<PackRowsArgs> h_pack; DeviceArray<PackRowsArgs> d_pack;
    std::vector<DenseArgs> h_dense; DeviceArray<DenseArgs> d_dense;     // [nfwd][P] then [ndx][P] (launch order)
    std::vector<BcLossArgs> h_loss; DeviceArray<BcLossArgs> d_loss;
    std::vector<BcHeadArgs> h_head; DeviceArray<BcHeadArgs> d_head;
    std::vector<DenseDwSmallGroup> h_dw; DeviceArray<DenseDwSmallGroup> d_dw;
    std::vector<ReduceAdamArgs> h_ra; DeviceArray<ReduceAdamArgs> d_ra;
    PinnedArray<BcStep> steps; SlotRing<STEP_SLOTS> step_ring;          // [STEP_SLOTS][P]
    PinnedArray<unsigned> seq;                                          // pinned word: the launch number published last
    DeviceArray<unsigned> ticket;
    uint64_t launches = 0;                                              // launch numbers given out so far (1-based)
    std::vector<bdr_replay*> last_buffers;                              // the buffers of the last accepted opt (distinctness checked once)
    GroupAct<BcActCall> act;                                            // group acting (group_act.hpp): static arguments, call words, staging areas

    size_t fwd_at(int i, size_t P) const { return (size_t)i * P; }
    size_t dx_at(int j, size_t P) const { return (size_t)(nfwd + j) * P; }   // j-th dX launch of the round

    hipError_t allocate(size_t P)
    {
        const int L = shape.n_layers;
        head = shape.form == BG_FORM_FUSED_MFMA ? 1 : 0;
        nfwd = head ? L - 1 : L;
        ndx = head ? L - 2 : L - 1;
        h_gather.resize(P); h_pack.resize(P); h_dense.resize((size_t)(nfwd + ndx) * P); h_loss.resize(P); h_head.resize(P); h_dw.resize(P); h_ra.resize(P);
        keys.resize(P);
        hipError_t e = device_array(d_gather, P);
        if (e == hipSuccess) e = device_array(d_pack, P);
        if (e == hipSuccess) e = device_array(d_dense, std::max<size_t>(h_dense.size(), 1));
        if (e == hipSuccess) e = device_array(d_loss, P);
        if (e == hipSuccess) e = device_array(d_head, P);
        if (e == hipSuccess) e = device_array(d_dw, P);
        if (e == hipSuccess) e = device_array(d_ra, P);
        if (e == hipSuccess) e = device_array(ticket, 1);
        if (e == hipSuccess) e = hipMemset(ticket.get(), 0, sizeof(unsigned));
        if (e == hipSuccess) e = pinned_array(steps, (size_t)STEP_SLOTS * P);
        if (e == hipSuccess) e = pinned_array(seq, 16);   // (one word, a cache line of its own)
        return e;
    }
    // member p's arguments into the staging arrays
    void stage(size_t p, size_t P, const BcMemberArgs& o)
    {
        const int L = shape.n_layers;
        h_gather[p] = o.gather; h_pack[p] = o.pack; h_loss[p] = o.loss; h_head[p] = o.head; h_dw[p] = o.dw; h_ra[p] = o.ra;
        for (int i = 0; i < nfwd; ++i) h_dense[fwd_at(i, P) + p] = o.fwd[i];
        for (int j = 0; j < ndx; ++j) h_dense[dx_at(j, P) + p] = o.dx[(head ? L - 2 : L - 1) - j];
    }
    hipError_t upload(size_t P)
    {
        hipError_t e = hipMemcpy(d_gather.get(), h_gather.data(), P * sizeof(GatherArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_pack.get(), h_pack.data(), P * sizeof(PackRowsArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess && !h_dense.empty()) e = hipMemcpy(d_dense.get(), h_dense.data(), h_dense.size() * sizeof(DenseArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_loss.get(), h_loss.data(), P * sizeof(BcLossArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_head.get(), h_head.data(), P * sizeof(BcHeadArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_dw.get(), h_dw.data(), P * sizeof(DenseDwSmallGroup), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_ra.get(), h_ra.data(), P * sizeof(ReduceAdamArgs), hipMemcpyHostToDevice);
        return e;
    }
    // one round's launches on the group's stream, grids from the plan; the last one publishes `seq_no`
    int32_t launch(size_t P, const BcStep* steps_dev, unsigned seq_no)
    {
        int fwd = 0, dx = 0;
        for (int n = 0; n < n_launches; ++n) {
            const BgLaunch& l = plan[n];
            const dim3 grid(l.gx, l.gy, l.gz), block(l.threads);
            switch (l.kernel) {
            case BG_K_GATHER:
                BDR_TRY(replay_gather_group(stream, d_gather.get(), steps_dev, (uint32_t)sizeof(BcStep), (uint32_t)P, (uint64_t)shape.batch, (uint64_t)shape.obs_dim * 4));
                break;
            case BG_K_PACK: hipLaunchKernelGGL(k_pack_rows_group, grid, block, 0, stream, (const BDR_CONST_AS PackRowsArgs*)d_pack.get()); break;
            case BG_K_FWD:
                hipLaunchKernelGGL(k_bc_dense_small_group<false>, grid, block, 0, stream, (const BDR_CONST_AS DenseArgs*)(d_dense.get() + fwd_at(fwd++, P)));
                break;
            case BG_K_LOSS: hipLaunchKernelGGL(k_bc_loss_group, grid, block, 0, stream, (const BDR_CONST_AS BcLossArgs*)d_loss.get()); break;
            case BG_K_HEAD:
                if (shape.act_dim <= 32) hipLaunchKernelGGL(k_bc_head_mfma_group<1>, grid, block, 0, stream, (const BDR_CONST_AS BcHeadArgs*)d_head.get());
                else hipLaunchKernelGGL(k_bc_head_mfma_group<2>, grid, block, 0, stream, (const BDR_CONST_AS BcHeadArgs*)d_head.get());
                break;
            case BG_K_DX:
                hipLaunchKernelGGL(k_bc_dense_small_group<true>, grid, block, 0, stream, (const BDR_CONST_AS DenseArgs*)(d_dense.get() + dx_at(dx++, P)));
                break;
            case BG_K_DW: hipLaunchKernelGGL(k_bc_dense_dw_small_group, grid, block, 0, stream, (const BDR_CONST_AS DenseDwSmallGroup*)d_dw.get()); break;
            case BG_K_REDUCE_ADAM:
                hipLaunchKernelGGL(k_bc_reduce_adam_group, grid, block, 0, stream, (const BDR_CONST_AS ReduceAdamArgs*)d_ra.get(), (const BDR_CONST_AS BcStep*)steps_dev,
                                   ticket.get(), seq.dev, seq_no);
                break;
            default: return fail(BDR_ERR_INVALID, "BC group round: launch %d of the plan names no kernel", n);
            }
            BDR_HIP(hipGetLastError());
        }
        return BDR_OK;
    }
};

namespace {

// every refusal of a grouped opt, before anything moves: Bc::opt's checks, and what the grouped gather covers
int32_t bc_group_check_buffers(bdr_bc_group* g, bdr_replay* const* buffers)
{
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        const Bc* m = g->members[p];
        const bdr_replay* r = buffers[p];
        BDR_REQUIRE(r, "member %u: null buffer", p);
        BDR_REQUIRE(!m->prof && !m->grad_comm, "member %u: profiling or a gradient communicator was switched on after the group was created", p);
        BDR_REQUIRE(r->obs_bytes == (uint64_t)m->O * 4 && r->act_bytes == (uint64_t)m->A * 4, "member %u: replay rows do not match BC obs/act dims (f32 rows)", p);
        BDR_REQUIRE(r->device == g->device, "member %u: its replay buffer lives on another device", p);
        BDR_REQUIRE(!r->per, "member %u: a prioritized buffer cannot be stepped by a BC group (the grouped gather covers the uniform ring)", p);
        BDR_REQUIRE(!r->frame_stack, "member %u: a single-frame store cannot be stepped by a BC group", p);
        BDR_REQUIRE(r->index_rng == BDR_RNG_STDRNG, "member %u: the grouped gather draws the StdRng index stream only", p);
        if (r->size == 0) return fail(BDR_ERR_EMPTY, "member %u: batch() on an empty replay buffer", p);
    }
    if (g->last_buffers.size() == P && memcmp(g->last_buffers.data(), buffers, P * sizeof(bdr_replay*)) == 0) return BDR_OK;
    std::vector<const bdr_replay*> s(buffers, buffers + P);   // workgroups run side by side: one bdr_replay (its batch arrays, its stream position) per member
    std::sort(s.begin(), s.end());
    const auto dup = std::adjacent_find(s.begin(), s.end());
    if (dup != s.end()) {
        uint32_t second = 0;
        for (uint32_t p = 0, seen = 0; p < P; ++p) if (buffers[p] == *dup && seen++ == 1) { second = p; break; }
        return fail(BDR_ERR_INVALID, "member %u: it shares its replay buffer with an earlier member: every member needs a bdr_replay of its own (a view of one ring will do)", second);
    }
    g->last_buffers.clear();
    return BDR_OK;
}

// one update round: per member what Bc::opt / Bc::update do on the host, then the round's launches, the last of which publishes its number
int32_t bc_group_round(bdr_bc_group* g, bdr_replay* const* buffers)
{
    const uint32_t P = (uint32_t)g->members.size();
    const uint64_t k = g->launches + 1;
    const auto slot = g->step_ring.next();
    if (slot.wait) {   // the slot's last reader has published (bounded: wait_seq_word)
        bool arrived = false;
        BDR_TRY(wait_seq_word(g->seq.host.get(), (unsigned)slot.wait, g->stream, std::chrono::steady_clock::now(), &arrived));
    }
    BcStep* steps = g->steps.host.get() + (size_t)slot.slot * P;
    bool dirty = false;
    for (uint32_t p = 0; p < P; ++p) {
        Bc* m = g->members[p];
        bdr_replay* r = buffers[p];
        const int bs = (int)m->cfg.batch_size;
        BDR_TRY(m->ensure_batch(bs));
        GatherArgs plan{};
        BDR_TRY(replay_sample_plan(r, bs, g->stream, &plan));   // the host half of replay_sample_on_stream; the rows are k_gather_group's
        m->step += 1;
        const AdamScalars sc = DenseAgent::opt_scalars(m->cfg.opt, m->cfg.lr, m->step);
        m->n_opts += 1;
        m->last_B = bs;
        bdr_bc_group::StaticKey& key = g->keys[p];
        if (!key.valid || key.batch_gen != m->batch_gen || key.r_uid != r->uid || key.r_batch_gen != r->batch_gen) {
            BcMemberArgs o;
            bc_member_static(m, bs, r, plan, o);
            BDR_REQUIRE(o.dw_grid == (int)g->plan[g->n_launches - 2].gx, "member %u: the weight-gradient grid (%d) differs from the plan's (%u)", p, o.dw_grid,
                        g->plan[g->n_launches - 2].gx);
            g->stage(p, P, o);
            key.valid = true; key.batch_gen = m->batch_gen; key.r_uid = r->uid; key.r_batch_gen = r->batch_gen;
            dirty = true;
        }
        steps[p] = BcStep{plan.word_pos, plan.size, sc};
    }
    if (dirty) {   // rare (first step, a reallocation, another ring): behind everything the stream still holds
        BDR_HIP(hipStreamSynchronize(g->stream));
        BDR_HIP(g->upload(P));
    }
    std::atomic_thread_fence(std::memory_order_release);
    // (should a launch fail, k is the number of whatever the group launches next - later than every reader of the slot)
    g->launches = k; g->step_ring.record(k);
    BDR_TRY(g->launch(P, g->steps.dev + (size_t)slot.slot * P, (unsigned)k));
    g->kernel_launches += (uint64_t)g->n_launches;
    return BDR_OK;
}

// what bdr_agent_opt does around opt(), for every member, then the round
int32_t bc_group_opt(bdr_bc_group* g, bdr_replay* const* buffers)
{
    BDR_HIP(hipSetDevice(g->device));
    BDR_TRY(bc_group_check_buffers(g, buffers));
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {   // asynchronous: what an earlier synchronising call of the member read back surfaces here
        Bc* m = g->members[p];
        unsigned w[bdr_agent::ERR_WORDS];
        m->err_mirror_read(w);
        BDR_TRY(m->err_report(w));
    }
    for (uint32_t p = 0; p < P; ++p) g->members[p]->last_replay_uid = buffers[p]->uid;
    BDR_TRY(bc_group_round(g, buffers));
    g->last_buffers.assign(buffers, buffers + P);
    return BDR_OK;
}

// Policy::sample of the selected members (members == nullptr: all of them) on n host rows each, ONE launch: group_act.hpp's call with
// what is BC's - the policy net on the member's arena, bc_act_out of its activation_out, no words beyond the common ones
struct BcActKind {
    using Call = BcActCall;
    const float* arena(const Bc* m) const { return m->p; }
    void write_static(const Bc* m, DenseActArgs& a) const
    {
        a.nl = (int)m->net.L.size();
        for (int l = 0; l < a.nl; ++l) a.L[l] = DenseActLayer{m->p + m->net.L[l].w, m->p + m->net.L[l].b, m->net.L[l].Kp, m->net.L[l].Np, m->net.L[l].relu};
        a.mode = DA_BC; a.kind = m->cfg.policy.activation_out;
    }
    void noise(const Bc*, int*, uint64_t*) const {}   // (no noise stream: nothing draws)
    void call_words(Bc*, BcActCall&, int, uint64_t, uint64_t) const {}
    hipError_t set_lds_attr(int teams) const
    {
        return teams == 2 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bc_act_group<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DA_LDS_MAX)
                          : hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bc_act_group<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DA_LDS_MAX);
    }
    void launch(int teams, dim3 grid, size_t lds, hipStream_t stream, const BDR_CONST_AS DenseActArgs* args, const BDR_CONST_AS BcActCall* calls,
                const BDR_CONST_AS unsigned* sel, unsigned* ticket, unsigned* seq_host, unsigned seq) const
    {
        if (teams == 2) hipLaunchKernelGGL(k_bc_act_group<2>, grid, dim3(512), lds, stream, args, calls, sel, ticket, seq_host, seq);
        else hipLaunchKernelGGL(k_bc_act_group<1>, grid, dim3(256), lds, stream, args, calls, sel, ticket, seq_host, seq);
    }
};
int32_t bc_group_sample(bdr_bc_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows,
                        const int32_t* dtypes, float* const* act_out)
{
    return group_act_sample(g, BcActKind{}, members, n_sel, norms, n, rows, dtypes, act_out);
}

}  // namespace

namespace bdr {
// the action width of a member, for the BC group evaluator's check of act_row_bytes (trainer.hip); 0: no such member
int bc_group_act_dim(const void* group, uint32_t member)
{
    const auto* g = static_cast<const bdr_bc_group*>(group);
    return g && member < g->members.size() ? g->members[member]->A : 0;
}
}  // namespace bdr

extern "C" {

int32_t bdr_bc_group_create(bdr_agent* const* agents, uint32_t n, bdr_bc_group** out)
{
    BDR_REQUIRE(agents && out, "null argument");
    BDR_REQUIRE(n >= 1 && n <= BG_MAX_MEMBERS, "a group has 1 .. 65535 members");
    std::vector<Bc*> ms;
    std::vector<BgMember> desc;
    for (uint32_t p = 0; p < n; ++p) {
        BDR_REQUIRE(agents[p], "member %u: null agent", p);
        BDR_REQUIRE(!strcmp(agents[p]->kind(), "bc"), "member %u cannot join a BC group: not a BC agent (kind %s)", p, agents[p]->kind());
        BDR_REQUIRE(!agents[p]->group, "member %u cannot join a BC group: already a member of a group", p);
        Bc* m = static_cast<Bc*>(agents[p]);
        ms.push_back(m);
        desc.push_back(BgMember{bc_shape(m), m->device, m->prof ? 1 : 0, m->grad_comm ? 1 : 0, m});
    }
    const char* why = nullptr;
    int kernel = -1;
    const int who = bg_group_refusal(desc.data(), n, &why, &kernel);
    if (who == BG_NO_MEMBER) return kernel >= 0 ? fail(BDR_ERR_INVALID, "%u members of this shape: %s (%s)", n, why, bg_kernel_name(kernel)) : fail(BDR_ERR_INVALID, "%s", why);
    BDR_REQUIRE(who == BG_OK, "member %d cannot join a BC group: %s", who, why);
    std::unique_ptr<bdr_bc_group> g(new bdr_bc_group());
    g->device = ms[0]->device;
    BDR_HIP(hipSetDevice(g->device));
    g->shape = desc[0].shape;
    g->n_launches = bg_round_plan(g->shape, n, g->plan);
    BDR_REQUIRE(g->n_launches == bg_launch_count(g->shape.n_layers, g->shape.form), "the BC group launch plan is incomplete");
    // (a failure below leaves nothing adopted: the partially built group releases what it holds)
    BDR_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    BDR_HIP(g->allocate(n));
    // adopt: the member's own stream is drained, retired and destroyed; the member enqueues on the group's stream from now on
    for (Bc* m : ms) BDR_HIP(hipStreamSynchronize(m->stream));
    for (Bc* m : ms) {
        hipStream_t old = m->stream;
        m->stream = g->stream; m->group = g.get();
        if (old) { stream_retire(old); (void)hipStreamDestroy(old); }
    }
    g->members = std::move(ms);
    *out = g.release();
    return BDR_OK;
}

int32_t bdr_bc_group_destroy(bdr_bc_group* g)
{
    if (!g) return BDR_OK;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->stream);
    for (Bc* m : g->members) {   // the group owns its members; their stream is the group's, destroyed once below
        m->group = nullptr; m->stream = nullptr;
        (void)bdr_agent_destroy(m);
    }
    delete g;   // retires and destroys the stream, then releases the buffers
    return BDR_OK;
}

int32_t bdr_bc_group_size(const bdr_bc_group* g, uint32_t* n)
{
    BDR_REQUIRE(g && n, "null argument");
    *n = (uint32_t)g->members.size();
    return BDR_OK;
}

int32_t bdr_bc_group_member(const bdr_bc_group* g, uint32_t i, bdr_agent** out)
{
    BDR_REQUIRE(g && out, "null argument");
    BDR_REQUIRE(i < g->members.size(), "member %u of a group of %u", i, (unsigned)g->members.size());
    *out = g->members[i];
    return BDR_OK;
}

int32_t bdr_bc_group_info(const bdr_bc_group* g, bdr_group_info* out)
{
    BDR_REQUIRE(g && out, "null argument");
    memset(out, 0, sizeof *out);
    out->form = BDR_GROUP_FORM_BC_LAYERS;
    out->n_members = (uint32_t)g->members.size();
    out->launches_per_round = (uint32_t)g->n_launches;
    out->kernel_launches = g->kernel_launches;
    return BDR_OK;
}

int32_t bdr_bc_group_opt(bdr_bc_group* g, bdr_replay* const* buffers)
{
    BDR_REQUIRE(g && buffers, "null argument");
    return bc_group_opt(g, buffers);
}

int32_t bdr_bc_group_opt_with_scalars(bdr_bc_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    BDR_REQUIRE(g && buffers && out && n_out, "null argument");
    BDR_REQUIRE(cap_per_member >= 1, "cap_per_member must be positive");
    BDR_TRY(bc_group_opt(g, buffers));
    BDR_HIP(hipStreamSynchronize(g->stream));   // the one synchronisation: every record() below finds the stream idle
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        Bc* m = g->members[p];
        int n = 0;
        m->rec_opt = true;
        const int32_t st = m->record(out + (size_t)p * cap_per_member, cap_per_member, &n);
        m->rec_opt = false;
        BDR_TRY(st);
        n_out[p] = n;
    }
    for (uint32_t p = 0; p < P; ++p) {   // the records are complete whatever the error words say about the step that produced them
        const int32_t st = g->members[p]->err_check();
        if (st != BDR_OK) { if (bdr::g_err_deferred) bdr::g_err_deferred = 2; return st; }
    }
    return BDR_OK;
}

int32_t bdr_bc_group_sample(bdr_bc_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    BDR_REQUIRE(g && rows && dtypes && act_out, "null argument");
    return bc_group_sample(g, nullptr, (uint32_t)g->members.size(), norms, n, rows, dtypes, act_out);
}

int32_t bdr_bc_group_sample_members(bdr_bc_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n,
                                    const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    BDR_REQUIRE(g && members && rows && dtypes && act_out, "null argument");
    return bc_group_sample(g, members, n_sel, norms, n, rows, dtypes, act_out);
}

int32_t bdr_bc_group_sync(bdr_bc_group* g)
{
    BDR_REQUIRE(g, "null group");
    BDR_HIP(hipSetDevice(g->device));
    BDR_HIP(hipStreamSynchronize(g->stream));
    for (Bc* m : g->members) {
        BDR_TRY(m->after_sync());
        BDR_TRY(m->err_check());
    }
    return BDR_OK;
}

}  // extern "C"
