// ================================================================================================
// A group of candle DQN agents in the Mlp form: Dqn::opt_ (dqn/base.rs:172-189) of every member in the launch sequence CandleDqn::opt
// enqueues for ONE member - the gather, k_cdqn_pack, the forward layers (the passes (p, obs), (p_tgt, next_obs) and - double_dqn -
// (p, next_obs) are the instances of one launch per layer), the TD launch, the input gradients, the grouped weight gradient, reduce +
// Adam with the soft update riding on it - with every launch serving ALL members: the member index is grid dimension y, the network
// instance of a forward launch grid dimension z, x stays the member's own grid (candle_dqn_group_plan.hpp has the rule and the grids):
// 2 L + 4 launches whatever P is.  A launch grouping, not an agent kind: the members stay ordinary candle DQN agents on the group's
// stream.  A part of candle_dqn.hip's translation unit (it needs CandleDqn and the bodies of its kernels), included where the code stands.
// Each entry runs the body of the kernel it groups (candle_dqn.hip, dense.hpp, replay.hip) on the member's entry of a device array, read
// in place through the constant address space: the member comes from blockIdx, so it is uniform and the entry's fields are scalar
// loads, as they are from the kernel-argument segment of the standalone kernel.  Same bodies, same bits.
//   k_cdqn_td_group      grid (1, P), 1024 threads: one workgroup per member runs cdqn_td_body - k_cdqn_td's body, operation for
//                        operation: candle::row_sum runs inside the workgroup, in its block order, over the member's rows only -
//                        with its own red[32] in LDS.  An out-of-range action raises the MEMBER's err[ERR_ACTION] and is clamped.
//   k_cdqn_pack_group    grid (ceil(B O / 256), P): cdqn_pack_body on the member's entry.
//   forward, dX, dW      dense_group.hpp's entries (k_dense_small_members_z, k_dense_dw_small_members), which states their bounds.
//   k_cdqn_reduce_adam_group   grid (ceil(arena / 4 / 256), P): the LAST reader of the step slot.  Per member it reads this step's
//                        AdamScalars, whether this step tracks (the member's own soft_update_interval; its own tau is a static word of
//                        its entry), the Adam step number, and the addresses of the member's poison word (err[ERR_ACTION]) and of its
//                        `applied` word; a member whose poison word is up is left alone - parameters, moments, target, gradient arena
//                        and `applied` - exactly as k_dense_reduce_adam leaves a lone agent alone; the others step.  Every thread
//                        reaches bg_group_done, which publishes the round's launch number.
//   k_cdqn_act_group<T>  Policy::sample's device part of the selected members in ONE launch: dense_act_body in its DA_EPI_DQN form -
//                        the Q rows and dqn_q_argmax of each row, DA_EPI_ALL's DA_DQN branch with every thread returning to the entry.
// Bounds of every new index: member = blockIdx.y < gridDim.y = P = the length of pack, td, gather, of every array of DenseRound and of
// a step slot (CdqnStep[P]); inside a member every index is the body's own, with the bounds of the standalone kernel (k_cdqn_td's
// header comment in candle_dqn.hip: rows b < B, columns j < A <= Np, dy rows of Np floats; k_cdqn_pack: t < B O).  Acting: y <
// gridDim.y = the number of selected members = the length of `sel`; sel[y] < P = the length of `args` and `calls` (checked by the host
// before anything is enqueued); the member's result block holds n i64 indices, then n * A floats: idx is written at m0 + r < n, out at
// (m0 + r) * A + j < n * A.
// Memory traffic is plain vector stores, the agent-scope atomicOr of the error word and the ticket's atomics: nothing new.
// The host half - the members' adoption, the static argument arrays and their keys, the step ring and its slot rule, the round,
// records, the push - is group_core.hpp's; the staging of the gather, dense, dW and reduce launches and the walk over the plan are
// dense_group.hpp's.  CandleDqnGroupKind below says what is the candle DQN's.
// The settle rule under a group.  fill_step does per member what CandleDqn::opt / update do on the host, in their order: opt_tracks()
// with the member's own soft_update_counter and interval, step += 1 and the Mark, opt_scalars, n_opts, last_B.  Every call of the
// group that synchronises (bdr_candle_dqn_group_sync, _opt_with_scalars) and every synchronising call of a member (record, its own
// opt_with_scalars, err_check's report) settle()s the member: a member whose reduce + Adam was skipped gets step, n_opts and
// soft_update_counter back as it does alone, is reported by member index, and the other members' rounds stay counted.
// Acting.  After the launch the host runs each selected member's own explorer (CandleDqn::explore) on what came back, in member
// order: one SmallRng stream per member across group calls, subset calls, the member's own calls and rounds; a member that is not
// selected draws nothing.  A lone member's sample_raw also reads its device error words before the explorer (acting_errors); a group
// call does not - P synchronising reads would undo the one launch -, so a pending error surfaces at the next synchronising call
// instead of stopping the acting call before it draws (include/border_amd.h says so).
#pragma once
#include "dense_group.hpp"
#include "group_core.hpp"
#include "candle_dqn_group_plan.hpp"

// the per-step words of one member: the gather's, then this step's optimizer scalars, whether it tracks, its Adam step number, and
// where the member's poison word and `applied` word are
struct CdqnStep {
    unsigned long long word_pos, size; AdamScalars adam[1]; int track; unsigned long long step;
    const unsigned* poison; unsigned long long* applied;
};
static_assert(offsetof(CdqnStep, word_pos) == offsetof(GatherStepWords, word_pos) && offsetof(CdqnStep, size) == offsetof(GatherStepWords, size),
              "the grouped gather reads the first two words of a member's CdqnStep");

namespace {

struct CdqnPackArgs { const float* obs; const float* next_obs; int O, Kp, B; float* x_o; float* x_no; };

// ---- the group entries: grid dimension y is the member -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cdqn_pack_group(const BDR_CONST_AS CdqnPackArgs* args)
{
    const BDR_CONST_AS CdqnPackArgs& a = args[blockIdx.y];
    cdqn_pack_body(a.obs, a.next_obs, a.O, a.Kp, a.B, a.x_o, a.x_no);
}
__global__ __launch_bounds__(1024) void k_cdqn_td_group(const BDR_CONST_AS CdqnTdArgs* args)
{
    __shared__ float red[32];
    cdqn_td_body(args[blockIdx.y], red);
}
// reduce + Adam (+ the soft update on the rounds the member tracks) of every member; the last reader of the slot
__global__ __launch_bounds__(256) void k_cdqn_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS CdqnStep* steps, unsigned* ticket,
                                                                unsigned* seq_host, unsigned seq)
{
    const BDR_CONST_AS CdqnStep& st = steps[blockIdx.y];
    const AdamScalars d = dg_step_scalars(st.adam[0]);
    const int track = st.track;
    const unsigned long long step = st.step;
    const unsigned* poison = st.poison;
    unsigned long long* applied = st.applied;
    if (!*poison) {   // (uniform per member: every thread of the member's workgroups reads the same word)
        if (blockIdx.x == 0 && threadIdx.x == 0) *applied = step;
        dense_reduce_adam_body(args[blockIdx.y], 0, d, track, 0);
    }
    bg_group_done(ticket, seq_host, seq);
}

// ---- group acting ----------------------------------------------------------------------------------------------------------------------
// the words of one member's call (group_act.hpp reads them by name); out: the Q rows [n][A], idx: the first-maximum indices [n]
struct CdqnActCall { const uint8_t* rows; unsigned long long row_stride; const float* mean; const float* std; float* out; long long* idx; int n, f64; };
template <int TEAMS>
__global__ __launch_bounds__(256 * TEAMS) void k_cdqn_act_group(const BDR_CONST_AS DenseActArgs* args, const BDR_CONST_AS CdqnActCall* calls,
                                                                const BDR_CONST_AS unsigned* sel, unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    extern __shared__ __attribute__((aligned(16))) float da_lds[];
    const unsigned member = sel[blockIdx.y];
    dense_act_body<TEAMS, DA_EPI_DQN>(args[member], calls[member], da_lds);
    __threadfence_system();   // this thread's result rows are in host memory before its workgroup counts
    bg_group_done(ticket, seq_host, seq);
}

CqShape cdqn_shape(const CandleDqn* m)
{
    CqShape s{};
    s.obs_dim = m->O; s.n_actions = m->A; s.batch = (int)m->cfg.batch_size; s.double_dqn = m->cfg.double_dqn ? 1 : 0;
    s.form = m->cnn_form() ? CQ_FORM_ATARI_CNN : CQ_FORM_MLP;
    s.net = dg_net_shape(m->net, m->cfg.qnet.activation_out);
    return s;
}

// ---- host: one member's static arguments, exactly what CandleDqn::update hands its launches --------------------------------------------
struct CdqnMemberArgs : DenseMemberArgs<1> {
    CdqnPackArgs pack;
    CdqnTdArgs td;
};

// (bs: the batch size; r: the member's ring or view; plan: replay_sample_plan's descriptor of this step)
void cdqn_member_static(CandleDqn* m, int bs, const bdr_replay* r, const GatherArgs& plan, CdqnMemberArgs& o)
{
    const MlpLayout& net = m->net;
    const int L = (int)net.L.size();
    const DenseLayer& last = net.L[L - 1];
    const bool dd = m->cfg.double_dqn != 0;
    o.dense.clear();
    o.gather = dg_gather_static(r, plan);
    o.pack = CdqnPackArgs{reinterpret_cast<const float*>(r->b_obs), reinterpret_cast<const float*>(r->b_next), m->O, net.L[0].Kp, bs, m->x_o, m->x_no};
    {
        const float* pp[3] = {m->p, m->p_tgt, m->p}; const float* xs[3] = {m->x_o, m->x_no, m->x_no}; std::vector<float*>* as[3] = {&m->a_on, &m->a_tg, &m->a_onn};
        dg_fwd_entries(o.dense, net, dd ? 3 : 2, pp, xs, as, bs);
    }
    {
        CdqnTdArgs& t = o.td;
        t = CdqnTdArgs{};
        t.q_on = m->a_on[L - 1]; t.q_tg = m->a_tg[L - 1]; t.q_on_next = dd ? m->a_onn[L - 1] : nullptr;
        t.Np = last.Np; t.A = m->A; t.B = bs; t.act = r->b_act; t.act_bytes = 8; t.reward = r->b_reward; t.term = r->b_term;
        t.gamma = (float)m->cfg.discount_factor; t.loss_kind = m->cfg.critic_loss; t.relu_out = last.relu; t.verbose = m->verbose() ? 1 : 0;
        t.dy = m->dy[L - 1]; t.pred = m->pr_pred; t.q_next = m->pr_qn; t.y = m->pr_y; t.tgt = m->pr_tgt; t.dpred = m->pr_dpred; t.lrow = m->lrow;
        t.scal = m->scal; t.err = m->dev_err;
    }
    {   // mlp_backward_step: the entry always names the target (whether a round tracks is a step word); poison, applied and the step
        // number are step words too and stay null here
        std::vector<float*>* acts[1] = {&m->a_on}; std::vector<float*>* dys[1] = {&m->dy};
        float* tg[1] = {m->p_tgt};
        dg_step_entries(o, CQ_NET_Q, net, 1, &m->p, &m->g, &m->m, &m->v, tg, m->x_o, acts, dys, m->part, 0, m->off, bs, net.total, m->cfg.tau, nullptr);
    }
}

// group acting: the Q-network on the member's arena, the DA_DQN epilogue; no device draws - the explorer runs on the host
struct CdqnActKind : GroupActEntry<CdqnActCall, k_cdqn_act_group<1>, k_cdqn_act_group<2>> {
    using Out = int64_t;
    const float* arena(const CandleDqn* m) const { return m->p; }
    void write_static(const CandleDqn* m, DenseActArgs& a) const
    {
        a.nl = (int)m->net.L.size();
        for (int l = 0; l < a.nl; ++l) a.L[l] = DenseActLayer{m->p + m->net.L[l].w, m->p + m->net.L[l].b, m->net.L[l].Kp, m->net.L[l].Np, m->net.L[l].relu};
        a.mode = DA_DQN; a.kind = BDR_ACTIVATION_NONE;
    }
    void noise(const CandleDqn*, int*, uint64_t*) const {}   // (no device noise stream: nothing draws there)
    int act_cols(const CqShape& s) const { return s.n_actions; }
    // a member's result block: n i64 indices, then n * A floats of Q rows; an even number of floats per row, so that every block of
    // the area is 8-byte aligned
    int res_cols(int A) const { return A + 2 + (A & 1); }
    void call_words(CandleDqn*, CdqnActCall& c, int, uint64_t, uint64_t) const
    {
        c.idx = reinterpret_cast<long long*>(c.out);
        c.out = c.out + 2 * (size_t)c.n;
    }
    // what came back -> the member's h_idx / h_q, then its own explorer (CandleDqn::explore), as its sample_raw ends
    int32_t result(CandleDqn* m, const float* block, uint64_t n, int A, int64_t* out) const
    {
        m->h_idx.resize(n); m->h_q.resize(n * (size_t)A);
        memcpy(m->h_idx.data(), block, n * 8);
        memcpy(m->h_q.data(), block + 2 * n, n * (size_t)A * 4);
        return m->explore(n, out, nullptr);
    }
};

// ---- what is the candle DQN's of the group core (group_core.hpp) -------------------------------------------------------------------------
struct CandleDqnGroupKind : DenseRound<1, CQ_K_DW, CQ_K_REDUCE_ADAM> {
    using Member = CandleDqn; using Shape = CqShape; using Launch = CqLaunch; using Step = CdqnStep; using MemberArgs = CdqnMemberArgs; using PlanMember = CqMember;
    using Act = CdqnActKind;
    static constexpr const char *KIND = "candle_dqn", *A = "a candle DQN", *NAME = "DQN (candle)", *CAP_MSG = "cap_per_member must be positive";
    static constexpr int MAX_LAUNCHES = CQ_MAX_LAUNCHES, K_GATHER = CQ_K_GATHER, FORM = BDR_GROUP_FORM_CANDLE_DQN_LAYERS, MIN_CAP = 1;
    static CqMember describe(const CandleDqn* m) { return CqMember{cdqn_shape(m), 1, m->cfg.n_updates_per_opt, m->device, m->prof ? 1 : 0, m->grad_comm ? 1 : 0, m}; }
    static int refusal(const CqMember* m, unsigned n, const char** why, int* kernel) { return cq_group_refusal(m, n, why, kernel); }
    static const char* kernel_name(int k) { return cq_kernel_name(k); }
    static int round_plan(const CqShape& s, unsigned P, CqLaunch* out) { return cq_round_plan(s, P, out); }
    static int launch_count(const CqShape& s) { return cq_launch_count(s.net.n_layers); }
    // the ring's action rows: ONE i64 per row (CandleDqn::opt's check)
    static uint64_t act_row_bytes(const CandleDqn*) { return 8; }
    // CandleDqn::opt / update on the host, in their order
    static CdqnStep fill_step(CandleDqn* m, int bs, const GatherArgs& plan)
    {
        CdqnStep st{};
        st.word_pos = plan.word_pos; st.size = plan.size;
        st.track = m->opt_tracks() ? 1 : 0;
        m->step += 1;
        m->marks.push_back(CandleDqn::Mark{m->step, m->opt_n0, m->opt_s0});
        if (m->marks.size() > 4096) m->marks.pop_front();
        st.adam[0] = DenseAgent::opt_scalars(m->cfg.opt, m->cfg.lr, m->step);
        st.step = m->step; st.poison = m->dev_err + bdr_agent::ERR_ACTION; st.applied = m->applied;
        m->n_opts += 1;
        m->last_B = bs;
        return st;
    }
    static void member_static(CandleDqn* m, int bs, const bdr_replay* r, const GatherArgs& plan, CdqnMemberArgs& o) { cdqn_member_static(m, bs, r, plan, o); }

    static constexpr DgReduceEntry<CdqnStep> RA[] = {k_cdqn_reduce_adam_group};
    StagedArray<CdqnPackArgs> pack; StagedArray<CdqnTdArgs> td;   // [P]
    hipError_t allocate(const CqShape& s, size_t P)
    {
        return allocate_round(cq_dense_launches(s.net.n_layers), P, pack, [&] { return td.resize(P); });
    }
    void stage(size_t p, size_t P, const CdqnMemberArgs& o)
    {
        stage_dense(p, P, o);
        pack[p] = o.pack; td[p] = o.td;
    }
    hipError_t upload() { return staged_upload(gather, pack, dense, td, dw, ra); }
    int32_t launch(const GroupCore<CandleDqnGroupKind>& g, size_t P, const CdqnStep* steps_dev, unsigned seq_no) const { return dg_round_launch(g, P, steps_dev, seq_no, *this); }
    int32_t launch_own(const CqLaunch& l, int n, size_t, dim3 grid, dim3 block, const BDR_CONST_AS CdqnStep*, hipStream_t stream) const
    {
        switch (l.kernel) {
        case CQ_K_PACK: hipLaunchKernelGGL(k_cdqn_pack_group, grid, block, 0, stream, (const BDR_CONST_AS CdqnPackArgs*)pack.d.get()); break;
        case CQ_K_TD: hipLaunchKernelGGL(k_cdqn_td_group, grid, block, 0, stream, (const BDR_CONST_AS CdqnTdArgs*)td.d.get()); break;
        default: return fail(BDR_ERR_INVALID, "DQN (candle) group round: launch %d of the plan names no kernel", n);
        }
        return BDR_OK;
    }
};

}  // namespace

struct bdr_candle_dqn_group : GroupCore<CandleDqnGroupKind> {};

namespace {

// a member's deferred report with the member named (the status and the deferred mark stay the member's)
int32_t cdqn_group_member_error(uint32_t p, int32_t st)
{
    const int deferred = bdr::g_err_deferred;
    const std::string msg = bdr::g_err;
    (void)fail(st, "member %u: %s", p, msg.c_str());
    bdr::g_err_deferred = deferred ? 2 : 0;
    return st;
}
// behind a synchronisation of the group's stream: every member settles, then the first member with an error word up is reported
int32_t cdqn_group_settle_and_check(bdr_candle_dqn_group* g)
{
    for (auto* m : g->members) BDR_TRY(m->after_sync());
    for (uint32_t p = 0; p < g->members.size(); ++p) {
        const int32_t st = g->members[p]->err_check();
        if (st != BDR_OK) return cdqn_group_member_error(p, st);
    }
    return BDR_OK;
}

}  // namespace

extern "C" {

int32_t bdr_candle_dqn_group_create(bdr_agent* const* agents, uint32_t n, bdr_candle_dqn_group** out) { return group_create(agents, n, out); }
int32_t bdr_candle_dqn_group_destroy(bdr_candle_dqn_group* g) { return group_destroy(g); }
int32_t bdr_candle_dqn_group_size(const bdr_candle_dqn_group* g, uint32_t* n) { return group_size(g, n); }
int32_t bdr_candle_dqn_group_member(const bdr_candle_dqn_group* g, uint32_t i, bdr_agent** out) { return group_member(g, i, out); }
int32_t bdr_candle_dqn_group_info(const bdr_candle_dqn_group* g, bdr_group_info* out) { return group_info(g, out); }
int32_t bdr_candle_dqn_group_opt(bdr_candle_dqn_group* g, bdr_replay* const* buffers) { return group_opt(g, buffers); }
// opt_with_record (dqn/base.rs:307-331) of every member: the round, ONE synchronisation, every member's record() - which settles it -
// then the error words, the first member that has one up named
int32_t bdr_candle_dqn_group_opt_with_scalars(bdr_candle_dqn_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    BDR_REQUIRE(g && buffers && out && n_out, "null argument");
    BDR_REQUIRE(cap_per_member >= CandleDqnGroupKind::MIN_CAP, "%s", CandleDqnGroupKind::CAP_MSG);
    BDR_TRY(group_opt(g, buffers));
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
    return cdqn_group_settle_and_check(g);
}
int32_t bdr_candle_dqn_group_sync(bdr_candle_dqn_group* g)
{
    BDR_REQUIRE(g, "null group");
    BDR_HIP(hipSetDevice(g->device));
    BDR_HIP(hipStreamSynchronize(g->stream));
    return cdqn_group_settle_and_check(g);
}
int32_t bdr_candle_dqn_group_sample(bdr_candle_dqn_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows, const int32_t* dtypes,
                                    int64_t* const* act_out)
{
    return group_sample(g, norms, n, rows, dtypes, act_out);
}
int32_t bdr_candle_dqn_group_sample_members(bdr_candle_dqn_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n,
                                            const void* const* rows, const int32_t* dtypes, int64_t* const* act_out)
{
    return group_sample_members(g, members, n_sel, norms, n, rows, dtypes, act_out);
}
// a test and diagnostic helper: the Q rows [n][A] the last acting call of the group that selected `member` brought back for it
// (the rows its explorer read)
int32_t bdr_candle_dqn_group_last_q(const bdr_candle_dqn_group* g, uint32_t member, float* q_out, uint64_t n_floats)
{
    BDR_REQUIRE(g && q_out, "null argument");
    BDR_REQUIRE(member < g->members.size(), "member %u of a group of %u", member, (unsigned)g->members.size());
    const CandleDqn* m = g->members[member];
    BDR_REQUIRE(n_floats == m->h_q.size() && n_floats > 0, "member %u holds %llu action values of its last acting call, not %llu", member,
                (unsigned long long)m->h_q.size(), (unsigned long long)n_floats);
    std::copy(m->h_q.begin(), m->h_q.end(), q_out);
    return BDR_OK;
}
// ExperienceBufferBase::push of n transitions per member in ONE launch (group_push: the action rows are copied as act_bytes = 8 bytes)
int32_t bdr_candle_dqn_group_push(bdr_candle_dqn_group* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs, const void* const* next_obs,
                                  const int32_t* obs_dtypes, const int64_t* const* act, const float* const* reward, const int8_t* const* is_terminated,
                                  const int8_t* const* is_truncated)
{
    return group_push(g, buffers, n, obs, next_obs, obs_dtypes, reinterpret_cast<const float* const*>(act), reward, is_terminated, is_truncated);
}
int32_t bdr_candle_dqn_group_push_max_rows(bdr_candle_dqn_group* g, bdr_replay* const* buffers, const int32_t* obs_dtypes, uint64_t* n_max)
{
    return group_push_max_rows(g, buffers, obs_dtypes, n_max);
}

}  // extern "C"
