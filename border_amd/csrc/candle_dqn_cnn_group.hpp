// ================================================================================================
// A group of candle DQN agents in the AtariCnn form: Dqn::opt_ (dqn/base.rs:172-189) of every member in the launch sequence
// CandleDqnCnn::opt / update_cnn enqueue for ONE member, every launch serving ALL members - 17 launches whatever P is
// (candle_dqn_cnn_group_plan.hpp has the rule, the order and the grids): the member index is grid dimension y of every launch.
// A launch grouping, not an agent kind.  It covers the UPDATE ROUND only: acting, push, evaluation, the compiled online loop and
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

// no acting for CNN members: the core's acting state stays empty
struct CdqnCnnNoAct { using Call = CdqnActCall; using Out = int64_t; };

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

}  // extern "C"
