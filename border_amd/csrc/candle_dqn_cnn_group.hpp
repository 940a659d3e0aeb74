// ================================================================================================
// A group of candle DQN agents in the AtariCnn form: Dqn::opt_ (dqn/base.rs:172-189) of every member in the launch sequence
// CandleDqnCnn::opt / update_cnn enqueue for ONE member, every launch serving ALL members - 17 launches whatever P is
// (candle_dqn_cnn_group_plan.hpp has the rule, the order and the grids): the member index is grid dimension y of every launch.
// A launch grouping, not an agent kind.  It covers the update round and ACTING (below); push, evaluation, the compiled online loop and
// copies between members are not built for CNN members.  The members stay ordinary agents on the group's stream - their own sample,
// qvalues, set_hyper and checkpoint calls keep working between rounds.  A part of candle_dqn.hip's translation unit.
//   trunk forward, dX, dW       conv_group.hpp's entries (k_conv1_img_members, k_igemm_members, k_igemm_red_members, k_conv1_dw_members),
//                               which states their bounds.
//   head forward, dX, dW        dense_group.hpp's entries (k_dense_small_members_z, k_dense_dw_small_members); l1's input gradient into
//                               dy3 under conv3's ReLU mask is one more dX entry (dg_step_entries' dx0 / mask0).
//   k_cdqn_td_group             candle_dqn_group.hpp's TD entry, unchanged.
//   k_cdqn_head_reduce_adam_group   grid (ceil(head arena / 4 / 256), P): k_cdqn_reduce_adam_group's body without the ticket - in this
//                               round the head's reduce + Adam is NOT the last reader of the slot.
//   k_cdqn_conv_reduce_adam_group   grid (ceil(conv floats / 4 / 32), P): cdqn_conv_reduce_adam_body (k_cdqn_conv_reduce_adam's) on the
//                               member's segments; per member it reads this step's AdamScalars, `track`, the step number and the
//                               addresses of the member's poison and `applied` words from the step slot.  The LAST reader of the slot:
//                               every thread reaches bg_group_done.
// A member whose poison word (err[ERR_ACTION], raised by the TD launch of the same round; only the host clears it, with the stream
// idle) is up is left alone by BOTH reduce + Adam launches - head and conv parameters, moments, targets, gradient arena, `applied` -;
// the others step.
// Bounds of every new index: member = blockIdx.y < gridDim.y = P = the length of td, cra, of every array of DenseRound and ConvRound
// and of a step slot (CdqnStep[P]); inside a member every index is the body's own with the standalone kernel's bounds
// (k_cdqn_conv_reduce_adam's header comment in candle_dqn.hip: i < n4, segment k <= 2, j < seg.n4, chunks c < seg.chunks).
// No workgroup waits for another: the only device-side rendezvous is the end-of-round ticket (group_done.hpp).
// The settle rule is the Mlp group's (candle_dqn_group.hpp): fill_step does per member what CandleDqnCnn::opt / update_cnn do on the
// host, in their order - opt_tracks(), step += 1 and the Mark, opt_scalars, n_opts, last_B -; every synchronising call of the group
// or of a member settle()s the member: a member whose reduce + Adam launches were skipped gets step, n_opts and soft_update_counter
// back, is reported by member index, and the other members' rounds stay counted.
// Acting.  Policy::sample (dqn/base.rs:202-230) of the selected members, each on its own n <= CAI_MAX_ROWS host frame stacks, in TWO
// launches whatever P is: k_cnn_act_trunk_group, grid (n, n_sel), and k_cnn_act_head_group, grid (16, CAI_L1_KS, n_sel)
// (cnn_act_img.hpp has the kernels and their bounds) - the members' own image acting path with the member as a grid dimension, same
// sums, same bits.  The host half is cdqn_cnn_group_act below:
//   static per member   a CnnActTrunkArgs and a CnnActHeadArgs in two device arrays [P], keyed on the member's parameter arena and
//                       rewritten when it has moved, behind a stream synchronise (group_act.hpp's rule); feat [P][32][3136] and, per
//                       member, partial tiles, h1, Q rows [32][A] and 17 counters (zeroed once; every launch leaves them zero) are
//                       the group's own device memory: a member's own img_feat, samp and probes are not touched.
//   per call            calls [P], sel [P], the staged rows and the results, ONE pinned, device-mapped area each; the selection, the
//                       offsets and the cap are group_act_plan.hpp's with a row of 7056 n_stack bytes (1764 n_stack words: every
//                       member's block is 16-byte aligned, the trunk stages 16-byte vectors) and a result row of A + 1 floats: the
//                       member's block is Q [n][A], then its n first-maximum indices as int32.
// The head launch takes the next number of the group's one counter - rounds and acting calls are ordered on the group's stream -
// and ends with the group's ticket; the host waits for that number (wait_seq_word), then runs every selected member's own explorer
// (CandleDqn::explore) in member order on what came back: Softmax reads the Q rows, epsilon-greedy and eval mode the indices;
// n_samples_act, n_samples_best_act and the epsilon counter move as they do alone, and group calls, rounds and the member's own
// bdr_agent_sample* calls continue ONE explorer stream.  Pending device error words are not read (candle_dqn_group.hpp's rule).
// Everything is checked before anything is staged, enqueued or drawn.
#pragma once
#include "candle_dqn_group.hpp"
#include "conv_group.hpp"

namespace {

// the static words of a member's conv reduce + Adam (s, track, poison, applied, step of the struct are this step's: the slot's)
__global__ __launch_bounds__(256) void k_cdqn_conv_reduce_adam_group(const BDR_CONST_AS CdqnConvAdamArgs* args, const BDR_CONST_AS CdqnStep* steps, unsigned* ticket,
                                                                     unsigned* seq_host, unsigned seq)
{
    __shared__ f32x4 red[8][32];
    const BDR_CONST_AS CdqnStep& st = steps[blockIdx.y];
    const AdamScalars d = dg_step_scalars(st.adam[0]);
    const int track = st.track;
    const unsigned long long step = st.step;
    const unsigned* poison = st.poison;
    unsigned long long* applied = st.applied;
    if (!*poison)   // (uniform per member: every thread of the member's workgroups reads the same word)
        cdqn_conv_reduce_adam_body(args[blockIdx.y], d, track, applied, step, red);
    bg_group_done(ticket, seq_host, seq);
}
// the head's reduce + Adam (+ the soft update on the rounds the member tracks); NOT the last reader of the slot here
__global__ __launch_bounds__(256) void k_cdqn_head_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS CdqnStep* steps, unsigned*, unsigned*,
                                                                     unsigned)
{
    const BDR_CONST_AS CdqnStep& st = steps[blockIdx.y];
    const AdamScalars d = dg_step_scalars(st.adam[0]);
    const int track = st.track;
    const unsigned long long step = st.step;
    const unsigned* poison = st.poison;
    unsigned long long* applied = st.applied;
    if (!*poison) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *applied = step;
        dense_reduce_adam_body(args[blockIdx.y], 0, d, track, 0);
    }
}

inline const CandleDqnCnn* cdqn_cnn(const CandleDqn* m) { return static_cast<const CandleDqnCnn*>(m); }
inline CandleDqnCnn* cdqn_cnn(CandleDqn* m) { return static_cast<CandleDqnCnn*>(m); }

// ---- host: one member's static arguments, exactly what CandleDqnCnn::update_cnn hands its launches -------------------------------------
struct CdqnCnnMemberArgs : DenseMemberArgs<1> {
    ConvMemberArgs conv;
    CdqnTdArgs td;
    CdqnConvAdamArgs cra;
};
void cdqn_cnn_member_static(CandleDqnCnn* m, int bs, const bdr_replay* r, const GatherArgs& plan, CdqnCnnMemberArgs& o)
{
    const MlpLayout& net = m->net;
    const int L = (int)net.L.size(), nz = m->cfg.double_dqn ? 3 : 2;
    const DenseLayer& last = net.L[L - 1];
    o.dense.clear();
    o.gather = dg_gather_static(r, plan);
    {
        const float* pp[3] = {m->p, m->p_tgt, m->p}; const uint8_t* rows[3] = {r->b_obs, r->b_next, r->b_next};
        cg_member_static(m->conv, nz, pp, rows, m->a1, m->a2, m->a3, m->dy3, m->dy2, m->dy1, m->part_conv, bs, m->B, o.conv);
        const float* hp[3] = {m->head(m->p), m->head(m->p_tgt), m->head(m->p)}; const float* xs[3] = {m->a3[0], m->a3[1], m->a3[2]};
        std::vector<float*>* as[3] = {&m->a_on, &m->a_tg, &m->a_onn};
        dg_fwd_entries(o.dense, net, nz, hp, xs, as, bs);
    }
    {
        CdqnTdArgs& t = o.td;
        t = CdqnTdArgs{};
        t.q_on = m->a_on[L - 1]; t.q_tg = m->a_tg[L - 1]; t.q_on_next = m->cfg.double_dqn ? m->a_onn[L - 1] : nullptr;
        t.Np = last.Np; t.A = m->A; t.B = bs; t.act = r->b_act; t.act_bytes = 8; t.reward = r->b_reward; t.term = r->b_term;
        t.gamma = (float)m->cfg.discount_factor; t.loss_kind = m->cfg.critic_loss; t.relu_out = 0; t.verbose = m->verbose() ? 1 : 0;
        t.dy = m->dy[L - 1]; t.pred = m->pr_pred; t.q_next = m->pr_qn; t.y = m->pr_y; t.tgt = m->pr_tgt; t.dpred = m->pr_dpred; t.lrow = m->lrow;
        t.scal = m->scal; t.err = m->dev_err;
    }
    {   // the head's mlp_backward_step with dx0 / mask0: the entry always names the target (whether a round tracks is a step word)
        std::vector<float*>* acts[1] = {&m->a_on}; std::vector<float*>* dys[1] = {&m->dy};
        float *hp = m->head(m->p), *hg = m->head(m->g), *hm = m->head(m->m), *hv = m->head(m->v), *ht[1] = {m->head(m->p_tgt)};
        float* dx0[1] = {m->dy3}; const float* mask0[1] = {m->a3[0]};
        dg_step_entries(o, CQC_NET_Q, net, 1, &hp, &hg, &hm, &hv, ht, m->a3[0], acts, dys, m->part, 0, m->off, bs, net.total, m->cfg.tau, nullptr, dx0, mask0);
    }
    {   // the segments in arena order, as trunk_backward's hook fills them
        CdqnConvAdamArgs& ra = o.cra;
        ra = CdqnConvAdamArgs{};
        for (int k = 0; k < 3; ++k) {
            const ConvDwLayer& l = o.conv.layer[k];
            ra.seg[k] = CdqnConvSeg{m->part_conv + l.off, l.stride, o.conv.dw_chunks[k], (unsigned)(l.w / 4), (unsigned)(l.n / 4), (unsigned)(l.n_weights / 4), l.wscale};
        }
        ra.p = m->p; ra.g = m->g; ra.m = m->m; ra.v = m->v; ra.tgt = m->p_tgt; ra.n4 = (unsigned)(m->conv_floats() / 4);
        ra.tau = (float)m->cfg.tau; ra.omt = (float)(1.0 - m->cfg.tau);
    }
}

// CNN members do not act through group_act.hpp's one launch over dense_act_body: the core's acting state stays empty
struct CdqnCnnNoAct { using Call = CdqnActCall; using Out = int64_t; };
// the state of cdqn_cnn_group_act
struct CdqnCnnGroupAct {
    std::vector<const float*> keys;                                                 // [P] the arena the static entries were written for (null: not yet)
    std::vector<CnnActTrunkArgs> h_trunk; DeviceArray<CnnActTrunkArgs> d_trunk;     // [P]
    std::vector<CnnActHeadArgs> h_head; DeviceArray<CnnActHeadArgs> d_head;         // [P]
    DeviceArray<float> feat;                                                        // [P][32][3136]
    DeviceArray<float> work;                                                        // [P][CAI_PART_FLOATS + 32 A] floats, then [P][CAI_COUNTERS] words
    PinnedArray<CnnActGroupCall> calls; PinnedArray<unsigned> sel;                  // [P], [P]
    PinnedArray<uint8_t> rows; size_t rows_cap = 0;                                 // bytes
    PinnedArray<float> res; size_t res_cap = 0;                                     // floats
};

// ---- what is this kind's of the group core (group_core.hpp) ----------------------------------------------------------------------------
struct CandleDqnCnnGroupKind : DenseRound<1, CQC_K_DW, CQC_K_REDUCE_ADAM> {
    using Member = CandleDqn; using Shape = CqcShape; using Launch = CqcLaunch; using Step = CdqnStep; using MemberArgs = CdqnCnnMemberArgs; using PlanMember = CqcMember;
    using Act = CdqnCnnNoAct;
    static constexpr const char *KIND = "candle_dqn", *A = "a candle DQN CNN", *NAME = "DQN (candle, AtariCnn)", *CAP_MSG = "cap_per_member must be positive";
    static constexpr int MAX_LAUNCHES = CQC_MAX_LAUNCHES, K_GATHER = CQC_K_GATHER, FORM = BDR_GROUP_FORM_CANDLE_DQN_CNN_LAYERS, MIN_CAP = 1;
    // (an Mlp-form agent has kind "candle_dqn" too: nothing of the AtariCnn form is read from it, and the rule refuses it by name)
    static CqcMember describe(const CandleDqn* m)
    {
        CqcMember d{};
        d.kind_cdqn_cnn = m->cnn_form() ? 1 : 0; d.n_updates = m->cfg.n_updates_per_opt; d.device = m->device; d.prof = m->prof ? 1 : 0; d.grad_comm = m->grad_comm ? 1 : 0;
        d.agent = m;
        if (!d.kind_cdqn_cnn) return d;
        const CandleDqnCnn* c = cdqn_cnn(m);
        d.split_arith = c->b3() ? 1 : 0;
        d.head_splitk = c->head_form == BDR_HEAD_FORM_SPLITK ? 1 : 0;
        d.head_bwd_fused = c->head_bwd_form == BDR_HEAD_BWD_FUSED ? 1 : 0;
        CqcShape& s = d.shape;
        s.n_stack = c->conv.ns; s.obs_dim = (int)(c->row_bytes() / 4); s.n_actions = m->A; s.batch = (int)m->cfg.batch_size; s.double_dqn = m->cfg.double_dqn ? 1 : 0;
        s.dxc3_kloop = m->dxc3_kloop ? 1 : 0;
        s.net = dg_net_shape(m->net, BDR_ACTIVATION_NONE);
        return d;
    }
    static int refusal(const CqcMember* m, unsigned n, const char** why, int* kernel) { return cqc_group_refusal(m, n, why, kernel); }
    static const char* kernel_name(int k) { return cqc_kernel_name(k); }
    static int round_plan(const CqcShape& s, unsigned P, CqcLaunch* out) { return cqc_round_plan(s, P, out); }
    static int launch_count(const CqcShape&) { return cqc_launch_count(); }
    static uint64_t act_row_bytes(const CandleDqn*) { return 8; }                                      // ONE i64 per row
    static uint64_t obs_row_bytes(const CandleDqn* m) { return (uint64_t)cdqn_cnn(m)->row_bytes(); }   // u8 rows of 84 * 84 * n_stack bytes
    // CandleDqnCnn::opt / update_cnn on the host, in their order
    static CdqnStep fill_step(CandleDqn* m, int bs, const GatherArgs& plan) { return CandleDqnGroupKind::fill_step(m, bs, plan); }
    static void member_static(CandleDqn* m, int bs, const bdr_replay* r, const GatherArgs& plan, CdqnCnnMemberArgs& o) { cdqn_cnn_member_static(cdqn_cnn(m), bs, r, plan, o); }

    static constexpr DgReduceEntry<CdqnStep> RA[] = {k_cdqn_head_reduce_adam_group};
    StagedArray<CdqnTdArgs> td; StagedArray<CdqnConvAdamArgs> cra; ConvRound conv;   // [P]
    unsigned* done_ticket = nullptr; unsigned* done_seq = nullptr; unsigned done_no = 0;   // the round in flight: what the last launch publishes
    CqcShape sh{};                                                                         // the group's one shape: which trunk entries a round launches
    CdqnCnnGroupAct img;                                                                   // group acting (cdqn_cnn_group_act)
    hipError_t allocate(const CqcShape& s, size_t P)
    {
        sh = s;
        return allocate_round(cqc_dense_launches(), P, td, [&] { const hipError_t e = conv.resize(P); return e == hipSuccess ? cra.resize(P) : e; });
    }
    void stage(size_t p, size_t P, const CdqnCnnMemberArgs& o)
    {
        stage_dense(p, P, o);
        td[p] = o.td; cra[p] = o.cra; conv.stage(p, o.conv);
    }
    hipError_t upload()
    {
        const hipError_t e = staged_upload(gather, dense, td, dw, ra, cra);
        return e == hipSuccess ? conv.upload() : e;
    }
    // the plan's grids against the member's: the head's (DenseRound), then the conv weight gradients' chunks of this batch
    int32_t check_static(const GpLaunch* plan, int n_launches, const CdqnCnnMemberArgs& o, uint32_t p) const
    {
        BDR_TRY((DenseRound<1, CQC_K_DW, CQC_K_REDUCE_ADAM>::check_static(plan, n_launches, o, p)));
        for (int n = 0; n < n_launches; ++n) {
            const int k = plan[n].kernel == CQC_K_CONV1_DW ? 0 : plan[n].kernel == CQC_K_CONV2_DW ? 1 : plan[n].kernel == CQC_K_CONV3_DW ? 2 : -1;
            if (k < 0) continue;
            const unsigned own = (unsigned)(o.conv.layer[k].wgs * o.conv.dw_chunks[k]);
            BDR_REQUIRE(own == plan[n].gx, "member %u: the weight-gradient grid of conv%d (%u) differs from the plan's (%u)", p, k + 1, own, plan[n].gx);
        }
        return BDR_OK;
    }
    int32_t launch(const GroupCore<CandleDqnCnnGroupKind>& g, size_t P, const CdqnStep* steps_dev, unsigned seq_no)
    {
        done_ticket = g.ticket.get(); done_seq = g.seq.dev; done_no = seq_no;
        return dg_round_launch(g, P, steps_dev, seq_no, *this);
    }
    int32_t launch_own(const CqcLaunch& l, int n, size_t, dim3 grid, dim3 block, const BDR_CONST_AS CdqnStep* st, hipStream_t stream) const;
};

}  // namespace

struct bdr_candle_dqn_cnn_group : GroupCore<CandleDqnCnnGroupKind> {};

namespace {

int32_t CandleDqnCnnGroupKind::launch_own(const CqcLaunch& l, int n, size_t, dim3 grid, dim3 block, const BDR_CONST_AS CdqnStep* st, hipStream_t stream) const
{
    switch (l.kernel) {
    case CQC_K_TD: hipLaunchKernelGGL(k_cdqn_td_group, grid, block, 0, stream, (const BDR_CONST_AS CdqnTdArgs*)td.d.get()); return BDR_OK;
    case CQC_K_CONV_REDUCE_ADAM:
        hipLaunchKernelGGL(k_cdqn_conv_reduce_adam_group, grid, block, 0, stream, (const BDR_CONST_AS CdqnConvAdamArgs*)cra.d.get(), st, done_ticket, done_seq, done_no);
        return BDR_OK;
    default: break;
    }
    // the trunk's launches (conv_group.hpp): the instantiation by the group's one shape
    const hipError_t err = cg_launch(conv, l.kernel, sh.n_stack, cqc_conv1_ipw(sh), sh.dxc3_kloop != 0, grid, block, stream);
    if (err == hipErrorInvalidValue) return fail(BDR_ERR_INVALID, "DQN (candle, AtariCnn) group round: launch %d of the plan names no kernel", n);
    BDR_HIP(err);
    return BDR_OK;
}

// behind a synchronisation of the group's stream: every member settles, then the first member with an error word up is reported
int32_t cdqn_cnn_group_settle_and_check(bdr_candle_dqn_cnn_group* g)
{
    for (auto* m : g->members) BDR_TRY(m->after_sync());
    for (uint32_t p = 0; p < g->members.size(); ++p) {
        const int32_t st = g->members[p]->err_check();
        if (st != BDR_OK) return cdqn_group_member_error(p, st);
    }
    return BDR_OK;
}
// what the grouped gather covers, by name, before anything is enqueued: u8 rings (and views of one ring) of the members' row width
int32_t cdqn_cnn_group_check_rings(const bdr_candle_dqn_cnn_group* g, bdr_replay* const* buffers)
{
    for (uint32_t p = 0; p < g->members.size(); ++p) {
        const bdr_replay* r = buffers[p];
        BDR_REQUIRE(r, "member %u: null buffer", p);
        BDR_REQUIRE(!r->frame_stack, "member %u: a frame-stack store cannot be stepped by a candle DQN CNN group (the grouped gather copies whole u8 rows)", p);
        BDR_REQUIRE(!r->per, "member %u: a prioritized buffer cannot be stepped by a candle DQN CNN group (the grouped gather covers the uniform ring)", p);
        const uint64_t rb = CandleDqnCnnGroupKind::obs_row_bytes(g->members[p]);
        BDR_REQUIRE(r->obs_bytes == rb, "member %u: replay rows of %llu bytes do not match DQN (candle, AtariCnn) u8 rows of 84 x 84 x n_stack = %llu bytes", p,
                    (unsigned long long)r->obs_bytes, (unsigned long long)rb);
    }
    return BDR_OK;
}


// Policy::sample of the selected members (members == nullptr: all of them) on n host frame stacks each: two launches, then the explorers
int32_t cdqn_cnn_group_act(bdr_candle_dqn_cnn_group* g, const uint32_t* members, uint32_t n_sel, uint64_t n, const uint8_t* const* rows, int64_t* const* act_out)
{
    CdqnCnnGroupAct& s = g->kind.img;
    const uint32_t P = (uint32_t)g->members.size();
    const GaSelect pick = ga_select(members, n_sel, P);
    BDR_REQUIRE(pick.refusal != GA_EMPTY, "the member list is empty");
    BDR_REQUIRE(pick.refusal != GA_RANGE, "member %u (entry %u of the member list) of a group of %u", members[pick.entry], pick.entry, P);
    BDR_REQUIRE(pick.refusal != GA_ORDER, "member %u (entry %u of the member list): the list must be strictly ascending", members[pick.entry], pick.entry);
    BDR_REQUIRE(pick.refusal != GA_COUNT, "%u rows for a group of %u", n_sel, P);
    const auto at = [&](uint32_t b) { return ga_member_at(members, b); };
    BDR_REQUIRE(n >= 1, "batch size out of range: a group acting call takes 1 .. %d frame stacks per member", CAI_MAX_ROWS);
    BDR_REQUIRE(n <= (uint64_t)CAI_MAX_ROWS, "%llu frame stacks per member: the grouped acting kernels serve one tile of %d rows per member; larger batches go "
                "through the members' own sample (bdr_agent_sample)", (unsigned long long)n, CAI_MAX_ROWS);
    for (uint32_t b = 0; b < n_sel; ++b) {
        BDR_REQUIRE(rows[at(b)], "member %u: null observation rows", at(b));
        BDR_REQUIRE(act_out[at(b)], "member %u: null act_out", at(b));
    }
    const int A = g->shape.n_actions, RC = A + 1, O = g->shape.obs_dim;   // (obs_dim: the u8 row in 4-byte words)
    const size_t row = ga_row_bytes(O, false);
    const std::vector<int> f64(P, 0);
    const GaPlan plan = ga_plan(members, n_sel, P, n, O, RC, f64.data());
    BDR_REQUIRE(plan.refusal == GA_OK, "member %u .. %u: %zu bytes of rows in one group acting call, more than the staging area's %zu: split the call", at(0),
                at(n_sel - 1), plan.staged, GA_STAGE_MAX);
    BDR_HIP(hipSetDevice(g->device));
    // ---- the areas (first call, growth) and the static arguments (first call, a moved arena): rare, behind whatever the stream holds
    const size_t W = CAI_PART_FLOATS + (size_t)32 * A;
    if (!s.d_head) {   // (d_head last: a failure before it leaves the first call to be made again)
        BDR_HIP(pinned_array(s.calls, P));
        BDR_HIP(pinned_array(s.sel, P));
        BDR_HIP(device_array(s.feat, (size_t)P * CAI_MAX_ROWS * 3136));
        BDR_HIP(device_array(s.work, P * W + (size_t)P * CAI_COUNTERS));
        BDR_HIP(hipMemset(s.work.get(), 0, (P * W + (size_t)P * CAI_COUNTERS) * 4));   // the counters start at zero and every launch leaves them so
        BDR_HIP(hipStreamSynchronize(nullptr));                                        // (the memset ran on the null stream, the kernels will not)
        s.h_trunk.assign(P, CnnActTrunkArgs{}); s.h_head.assign(P, CnnActHeadArgs{});
        s.keys.assign(P, nullptr);
        BDR_HIP(device_array(s.d_trunk, P));
        BDR_HIP(device_array(s.d_head, P));
    }
    if (plan.staged > s.rows_cap) {
        BDR_HIP(hipStreamSynchronize(g->stream));
        s.rows_cap = 0;
        BDR_HIP(pinned_array(s.rows, plan.staged));
        s.rows_cap = plan.staged;
    }
    if (plan.res_floats > s.res_cap) {
        BDR_HIP(hipStreamSynchronize(g->stream));
        s.res_cap = 0;
        BDR_HIP(pinned_array(s.res, plan.res_floats));
        s.res_cap = plan.res_floats;
    }
    bool dirty = false;
    for (uint32_t b = 0; b < n_sel; ++b) {
        const uint32_t p = at(b);
        const CandleDqnCnn* m = cdqn_cnn(g->members[p]);
        if (s.keys[p] == m->p) continue;
        const Arena& cv = m->conv;
        const DenseLayer &l1 = m->net.L[0], &l2 = m->net.L[1];
        const float* hp = m->head(m->p);
        float* work = s.work.get() + p * W;
        s.h_trunk[p] = CnnActTrunkArgs{nullptr, row, cv.ns, 1, m->p + cv.w1, m->p + cv.b1, m->p + cv.w2, m->p + cv.b2, m->p + cv.w3, m->p + cv.b3, s.feat.get()};
        s.h_head[p] = CnnActHeadArgs{s.feat.get(), hp + l1.w, hp + l1.b, hp + l2.w, hp + l2.b, l2.Np, work,
                                     reinterpret_cast<unsigned*>(s.work.get() + P * W) + (size_t)p * CAI_COUNTERS, 0, A, work + CAI_PART_FLOATS, nullptr};
        s.keys[p] = m->p;
        dirty = true;
    }
    if (dirty) {
        hipError_t e = hipStreamSynchronize(g->stream);
        if (e == hipSuccess) e = hipMemcpy(s.d_trunk.get(), s.h_trunk.data(), (size_t)P * sizeof(CnnActTrunkArgs), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s.d_head.get(), s.h_head.data(), (size_t)P * sizeof(CnnActHeadArgs), hipMemcpyHostToDevice);
        if (e != hipSuccess) s.keys.assign(P, nullptr);   // (nothing is known to be on the device: the next call writes it again)
        BDR_HIP(e);
    }
    // ---- this call's words, rows and selection
    for (uint32_t b = 0; b < n_sel; ++b) {
        const uint32_t p = at(b);
        memcpy(s.rows.host.get() + plan.row_off[b], rows[p], (size_t)n * row);
        s.calls.host.get()[p] = CnnActGroupCall{s.rows.dev + plan.row_off[b], s.res.dev + plan.res_off[b]};
        s.sel.host.get()[b] = p;
    }
    std::atomic_thread_fence(std::memory_order_release);
    // the head launch takes the next number of the group's one counter: opt rounds and acting calls are ordered on the group's stream
    const uint64_t k = g->launches + 1;
    g->launches = k;
    BDR_HIP(launch_cnn_act_trunk_group(g->stream, (int)n, n_sel, s.d_trunk.get(), s.calls.dev, s.sel.dev));
    g->kernel_launches += 1;
    BDR_HIP(launch_cnn_act_head_group(g->stream, (int)n, n_sel, s.d_head.get(), s.calls.dev, s.sel.dev, CnnActGroupDone{g->ticket.get(), g->seq.dev, (unsigned)k}));
    g->kernel_launches += 1;
    bool arrived = false;
    BDR_TRY(wait_seq_word(g->seq.host.get(), (unsigned)k, g->stream, std::chrono::steady_clock::now(), &arrived));
    if (!arrived) return fail(BDR_ERR_HIP, "the actions of a group acting call never arrived in host memory");
    std::atomic_thread_fence(std::memory_order_acquire);
    // what came back -> the member's h_q / h_idx, then its own explorer, as its sample ends
    for (uint32_t b = 0; b < n_sel; ++b) {
        CandleDqn* m = g->members[at(b)];
        const float* block = s.res.host.get() + plan.res_off[b];
        const int32_t* idx = reinterpret_cast<const int32_t*>(block + (size_t)n * A);
        m->h_q.assign(block, block + (size_t)n * A);
        m->h_idx.assign(idx, idx + n);
        BDR_TRY(m->explore(n, act_out[at(b)], nullptr));
    }
    return BDR_OK;
}

}  // namespace

extern "C" {

int32_t bdr_candle_dqn_cnn_group_create(bdr_agent* const* agents, uint32_t n, bdr_candle_dqn_cnn_group** out)
{ return group_create(agents, n, out); }
int32_t bdr_candle_dqn_cnn_group_destroy(bdr_candle_dqn_cnn_group* g) { return group_destroy(g); }
int32_t bdr_candle_dqn_cnn_group_size(const bdr_candle_dqn_cnn_group* g, uint32_t* n) { return group_size(g, n); }
int32_t bdr_candle_dqn_cnn_group_member(const bdr_candle_dqn_cnn_group* g, uint32_t i, bdr_agent** out) { return group_member(g, i, out); }
int32_t bdr_candle_dqn_cnn_group_info(const bdr_candle_dqn_cnn_group* g, bdr_group_info* out) { return group_info(g, out); }
int32_t bdr_candle_dqn_cnn_group_opt(bdr_candle_dqn_cnn_group* g, bdr_replay* const* buffers)
{
    BDR_REQUIRE(g && buffers, "null argument");
    BDR_TRY(cdqn_cnn_group_check_rings(g, buffers));
    return group_opt(g, buffers);
}
// opt_with_record (dqn/base.rs:307-331) of every member: the round, ONE synchronisation, every member's record() - which settles it -
// then the error words, the first member that has one up named
int32_t bdr_candle_dqn_cnn_group_opt_with_record(bdr_candle_dqn_cnn_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    BDR_REQUIRE(g && buffers && out && n_out, "null argument");
    BDR_REQUIRE(cap_per_member >= CandleDqnCnnGroupKind::MIN_CAP, "%s", CandleDqnCnnGroupKind::CAP_MSG);
    BDR_TRY(bdr_candle_dqn_cnn_group_opt(g, buffers));
    BDR_HIP(hipStreamSynchronize(g->stream));
    const uint32_t P = (uint32_t)g->members.size();
    for (uint32_t p = 0; p < P; ++p) {
        CandleDqn* m = g->members[p];
        int n = 0;
        m->rec_opt = true;
        const int32_t st = m->record(out + (size_t)p * cap_per_member, cap_per_member, &n);
        m->rec_opt = false;
        BDR_TRY(st);
        n_out[p] = n;
    }
    return cdqn_cnn_group_settle_and_check(g);
}
int32_t bdr_candle_dqn_cnn_group_sync(bdr_candle_dqn_cnn_group* g)
{
    BDR_REQUIRE(g, "null group");
    BDR_HIP(hipSetDevice(g->device));
    BDR_HIP(hipStreamSynchronize(g->stream));
    return cdqn_cnn_group_settle_and_check(g);
}

// Policy::sample (dqn/base.rs:202-230) of every member / of the members `members` on n host u8 frame stacks each: two launches
int32_t bdr_candle_dqn_cnn_group_sample(bdr_candle_dqn_cnn_group* g, uint64_t n, const uint8_t* const* rows, int64_t* const* act_out)
{
    BDR_REQUIRE(g && rows && act_out, "null argument");
    return cdqn_cnn_group_act(g, nullptr, (uint32_t)g->members.size(), n, rows, act_out);
}
int32_t bdr_candle_dqn_cnn_group_sample_members(bdr_candle_dqn_cnn_group* g, const uint32_t* members, uint32_t n_sel, uint64_t n, const uint8_t* const* rows,
                                                int64_t* const* act_out)
{
    BDR_REQUIRE(g && members && rows && act_out, "null argument");
    return cdqn_cnn_group_act(g, members, n_sel, n, rows, act_out);
}
// a test and diagnostic helper: the Q rows [n][A] the last acting call of the group that selected `member` brought back for it -
// the member's h_q, which its own sample / qvalues calls overwrite: valid until the member acts alone
int32_t bdr_candle_dqn_cnn_group_last_q(const bdr_candle_dqn_cnn_group* g, uint32_t member, float* q_out, uint64_t n_floats)
{
    BDR_REQUIRE(g && q_out, "null argument");
    BDR_REQUIRE(member < g->members.size(), "member %u of a group of %u", member, (unsigned)g->members.size());
    const CandleDqn* m = g->members[member];
    BDR_REQUIRE(n_floats == m->h_q.size() && n_floats > 0, "member %u holds %llu action values of its last acting call, not %llu", member,
                (unsigned long long)m->h_q.size(), (unsigned long long)n_floats);
    std::copy(m->h_q.begin(), m->h_q.end(), q_out);
    return BDR_OK;
}

}  // extern "C"
