// ================================================================================================
// A group of IQL agents: Iql::opt_ (iql/base.rs:157-188) of every member in the launch sequence Iql::update enqueues for ONE member -
// gather, pack, the critics', actor's and value's forwards, the value loss and step, V'(obs) | V'(next_obs), the critic loss and the
// critics' step with the soft update riding on it, the target critics again, the actor loss and the actor's step - with every launch
// serving ALL members: the member index is grid dimension y, the network instance (where the standalone launch has one) stays grid
// dimension z, x stays the member's own grid (iql_group_plan.hpp has the rule and the grids).  A launch grouping, not an agent kind:
// the members stay ordinary IQL agents on the group's stream.  A part of iql.hip's translation unit (it needs Iql and the bodies of
// IQL's kernels), included where the code stands.
// Each entry runs the body of the kernel it groups (iql.hip, dense.hpp, replay.hip) on the member's entry of a device array, read in
// place through the constant address space: member and instance come from blockIdx, so they are uniform and the entry's fields are
// scalar loads, as they are from the kernel-argument segment of the standalone kernel.  Same bodies, same bits.  The three loss kernels
// are one workgroup per member: candle::row_sum / row_max run inside that workgroup, in their block order, over the member's rows only.
// The host half - the members' adoption, the static argument arrays and their keys, the step ring and its slot rule, the round, records,
// sync - is group_core.hpp's, shared with the BC group; IqlGroupKind below says what is IQL's.  Per step a member has an IqlStep: the
// gather reads word_pos and size (GatherStepWords at its start), the three reduce + Adam launches its three AdamScalars.  The ACTOR's
// reduce + Adam is the LAST launch of a round that reads the slot, so it alone ends with the ticket and publishes the round's launch
// number (bg_group_done - all workgroups of its three-dimensional grid counted, behind a barrier every thread reaches:
// dense_reduce_adam_body returns early for threads past the arena, to the entry, not out of the kernel).
// Bounds of every new index:
//   member = blockIdx.y < gridDim.y = P = the length of gather, pack, vloss, closs, aloss and of a step slot;
//   z = blockIdx.z < gridDim.z = nz <= 4 = the instances of a DenseGroupEntry and of a ReduceAdamArgs (2 n_critics <= 4 is a condition
//   of the group);
//   the i-th forward / dX launch of the round (stream order) is handed dense + i * P and reads entry i * P + member, i < ndense =
//   ig_dense_launches: the array holds ndense * P entries; the weight-gradient and reduce + Adam launches of network n (value 0,
//   critic 1, actor 2) are handed dw + n * P / ra + n * P: 3 P entries each; NET < 3 = the AdamScalars of an IqlStep;
//   inside a member every index is the body's own, with the bounds of the standalone kernel.
// Acting: Policy::sample of the selected members in ONE launch of k_candle_act_group (candle_act_group.hpp, which states the bounds of
// its indices) through group_act.hpp, the host half BC's group shares; IqlActKind below is CandleActKind of an Iql.
#pragma once
#include "dense_group.hpp"
#include "candle_act_group.hpp"
#include "group_core.hpp"
#include "iql_group_plan.hpp"

static_assert(IG_DW_GROUP == DW_GROUP && IG_RA_SEGS == RA_SEGS && IG_MAXZ == DG_MAXZ && IG_SHAPE_LAYERS >= BDR_MAX_UNITS + 1, "iql_group_plan.hpp restates these limits");

// the per-step words of one member: the gather's, then the optimizer scalars of value, critics and actor (IgNetId's order)
struct IqlStep { unsigned long long word_pos, size; AdamScalars adam[3]; };
static_assert(offsetof(IqlStep, word_pos) == offsetof(GatherStepWords, word_pos) && offsetof(IqlStep, size) == offsetof(GatherStepWords, size),
              "the grouped gather reads the first two words of a member's IqlStep");
static_assert(IG_NET_VALUE == 0 && IG_NET_CRITIC == 1 && IG_NET_ACTOR == 2, "IqlStep::adam and the dW / reduce argument arrays are indexed by IgNetId");

namespace {

// ---- the group entries: grid dimension y is the member -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iql_pack_group(const BDR_CONST_AS IqlPackArgs* args) { iql_pack_body(args[blockIdx.y]); }
__global__ __launch_bounds__(1024) void k_iql_value_loss_group(const BDR_CONST_AS IqlValueArgs* args)
{
    __shared__ float red[32];
    iql_value_loss_body(args[blockIdx.y], red);
}
__global__ __launch_bounds__(1024) void k_iql_critic_loss_group(const BDR_CONST_AS IqlCriticArgs* args)
{
    __shared__ float red[32];
    iql_critic_loss_body(args[blockIdx.y], red);
}
__global__ __launch_bounds__(1024) void k_iql_actor_loss_group(const BDR_CONST_AS IqlActorArgs* args)
{
    __shared__ float red[32];
    iql_actor_loss_body(args[blockIdx.y], red);
}
// reduce + Adam of network NET of every member, instance z = blockIdx.z: the optimizer scalars of this step come from the member's
// staging slot; the critics track their targets at the member's own tau (a.tau / a.omt of its entry); the actor's is the last reader of
// the slot and publishes
template <int NET>
__global__ __launch_bounds__(256) void k_iql_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS IqlStep* steps, unsigned* ticket,
                                                               unsigned* seq_host, unsigned seq)
{
    const BDR_CONST_AS AdamScalars& s = steps[blockIdx.y].adam[NET];
    AdamScalars d;   // field by field: static indices, registers
    d.b1 = s.b1; d.omb1 = s.omb1; d.b2 = s.b2; d.omb2 = s.omb2; d.sqrt_bc2 = s.sqrt_bc2; d.eps = s.eps; d.neg_step = s.neg_step; d.wd_mul = s.wd_mul;
    dense_reduce_adam_body(args[blockIdx.y], (int)blockIdx.z, d, NET == IG_NET_CRITIC ? 1 : 0, 0);
    if constexpr (NET == IG_NET_ACTOR) bg_group_done(ticket, seq_host, seq);
}

IgShape iql_shape(const Iql* m)
{
    IgShape s{};
    s.obs_dim = m->O; s.act_dim = m->A; s.batch = (int)m->cfg.batch_size; s.n_critics = m->NC;
    s.value = dg_net_shape(m->vn, m->cfg.value.activation_out);
    s.critic = dg_net_shape(m->qn, m->cfg.critic.activation_out);
    s.actor = dg_net_shape(m->pn, m->cfg.actor.activation_out);
    return s;
}

// ---- host: one member's static arguments, exactly what Iql::update hands its launches (the dense, dX, dW and reduce entries of a
// network: dense_group.hpp's dg_fwd_entries / dg_step_entries) ---------------------------------------------------------------------------
struct IqlMemberArgs {
    GatherArgs gather; IqlPackArgs pack;
    std::vector<DenseGroupEntry> dense;   // the forward and dX launches in stream order
    IqlValueArgs vloss; IqlCriticArgs closs; IqlActorArgs aloss;
    DenseDwSmallGroup dw[3]; int dw_grid[3];   // by IgNetId
    ReduceAdamArgs ra[3];
};

// (bs: the batch size; r: the member's ring or view; plan: replay_sample_plan's descriptor of this step)
void iql_member_static(Iql* m, int bs, const bdr_replay* r, const GatherArgs& plan, IqlMemberArgs& o)
{
    const bdr_iql_config& cfg = m->cfg;
    const int NC = m->NC, O = m->O, A = m->A;
    const MlpLayout &qn = m->qn, &vn = m->vn, &pn = m->pn;
    const int Lq = (int)qn.L.size(), Lv = (int)vn.L.size(), Lp = (int)pn.L.size();
    const int ldq = qn.L[Lq - 1].Np, ldv = vn.L[Lv - 1].Np;
    const float* obs = reinterpret_cast<const float*>(r->b_obs);
    const float* next_obs = reinterpret_cast<const float*>(r->b_next);
    const float* act = reinterpret_cast<const float*>(r->b_act);
    o.dense.clear();
    // the gather: k_gather's arguments as replay_sample_on_stream sets them (word_pos and size are this step's, read from the slot)
    o.gather = plan;
    replay_gather_shape(r->obs_bytes, &o.gather.chunks, &o.gather.vec_per_chunk);
    o.gather.word_pos = 0; o.gather.size = 0;
    o.pack = IqlPackArgs{obs, next_obs, act, O, A, bs, m->x_o, m->x_no, vn.L[0].Kp, m->xq, qn.L[0].Kp};
    // target and online critics: one forward of 2 NC networks
    {
        const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
        for (int i = 0; i < NC; ++i) { params[i] = m->q_t[i]; x[i] = m->xq; acts[i] = &m->t_act[i]; params[NC + i] = m->q_p[i]; x[NC + i] = m->xq; acts[NC + i] = &m->c_act[i]; }
        dg_fwd_entries(o.dense, qn, 2 * NC, params, x, acts, bs);
    }
    { const float* pp[1] = {m->pi_p}; const float* x[1] = {m->x_o}; std::vector<float*>* acts[1] = {&m->p_act}; dg_fwd_entries(o.dense, pn, 1, pp, x, acts, bs); }
    // ---- update_value
    { const float* pp[1] = {m->v_p}; const float* x[1] = {m->x_o}; std::vector<float*>* acts[1] = {&m->v_act}; dg_fwd_entries(o.dense, vn, 1, pp, x, acts, bs); }
    {
        IqlValueArgs& p = o.vloss;
        p = IqlValueArgs{};
        for (int i = 0; i < NC; ++i) p.qt[i] = m->t_act[i][Lq - 1];
        p.ldq = ldq; p.NC = NC; p.v = m->v_act[Lv - 1]; p.dv = m->v_dy[Lv - 1]; p.ldv = ldv; p.relu_out = vn.L[Lv - 1].relu;
        p.tau = (float)cfg.tau_iql; p.q_min = m->pr_qmin1; p.v_out = m->pr_v; p.u_out = m->pr_u; p.loss = m->scal; p.accumulate = 0; p.B = bs;
    }
    {
        std::vector<float*>* acts[1] = {&m->v_act}; std::vector<float*>* dys[1] = {&m->v_dy};
        dg_step_entries(o, IG_NET_VALUE, vn, 1, &m->v_p, &m->v_g, &m->v_m, &m->v_v, nullptr, m->x_o, acts, dys, m->v_part, 0, m->v_off, bs, vn.total, cfg.critic_tau, nullptr);
    }
    // ---- update_critic
    {
        const float* pp[2] = {m->v_p, m->v_p}; const float* x[2] = {m->x_o, m->x_no}; std::vector<float*>* acts[2] = {&m->vo_act, &m->vn_act};
        dg_fwd_entries(o.dense, vn, 2, pp, x, acts, bs);
    }
    {
        IqlCriticArgs& p = o.closs;
        p = IqlCriticArgs{};
        for (int i = 0; i < NC; ++i) { p.q[i] = m->c_act[i][Lq - 1]; p.dq[i] = m->c_dy[i][Lq - 1]; }
        p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu; p.vn = m->vn_act[Lv - 1]; p.ldv = ldv;
        p.reward = r->b_reward; p.term = r->b_term; p.trunc = r->b_trunc; p.gamma = (float)cfg.gamma; p.tgt = m->pr_tgt; p.v_next = m->pr_vnext;
        p.loss_kind = cfg.critic_loss; p.loss = m->scal + 1; p.accumulate = 0; p.B = bs;
    }
    {
        std::vector<float*>* acts[4]; std::vector<float*>* dys[4];
        for (int i = 0; i < NC; ++i) { acts[i] = &m->c_act[i]; dys[i] = &m->c_dy[i]; }
        dg_step_entries(o, IG_NET_CRITIC, qn, NC, m->q_p, m->q_g, m->q_m, m->q_v, m->q_t, m->xq, acts, dys, m->q_part, m->q_part_stride, m->q_off, bs, qn.total,
                         cfg.critic_tau, nullptr);
    }
    // ---- update_actor
    {
        const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
        for (int i = 0; i < NC; ++i) { params[i] = m->q_t[i]; x[i] = m->xq; acts[i] = &m->t_act[i]; }
        dg_fwd_entries(o.dense, qn, NC, params, x, acts, bs);
    }
    {
        IqlActorArgs& p = o.aloss;
        p = IqlActorArgs{};
        for (int i = 0; i < NC; ++i) p.qt[i] = m->t_act[i][Lq - 1];
        p.ldq = ldq; p.NC = NC; p.vo = m->vo_act[Lv - 1]; p.ldv = ldv;
        p.mean = m->p_act[Lp - 1]; p.ldm = pn.L[Lp - 1].Np; p.head2 = m->pi_p + m->h2_off; p.act = act; p.A = A;
        p.lo = (float)cfg.min_log_std; p.hi = (float)cfg.max_log_std; p.tanh_limit = cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
        p.scale = (float)cfg.action_scale; p.inv_lambda = (float)cfg.inv_lambda; p.exp_adv_max = (float)cfg.exp_adv_max; p.softmax = cfg.adv_softmax ? 1 : 0;
        p.q_min = m->pr_qmin3; p.w = m->pr_w; p.logp = m->pr_logp; p.gmean = m->p_dy[Lp - 1]; p.gh2 = m->h2_part;
        p.loss = m->scal + 2; p.accumulate = 0; p.B = bs;
    }
    {
        std::vector<float*>* acts[1] = {&m->p_act}; std::vector<float*>* dys[1] = {&m->p_dy};
        const DenseReduceSeg h2seg{m->h2_part, (size_t)pad64(A), 1, (unsigned)(m->h2_off / 4), (unsigned)(pad64(A) / 4)};
        dg_step_entries(o, IG_NET_ACTOR, pn, 1, &m->pi_p, &m->pi_g, &m->pi_m, &m->pi_v, nullptr, m->x_o, acts, dys, m->pi_part, 0, m->pi_off, bs, m->pi_total,
                         cfg.critic_tau, &h2seg);
    }
}

// ---- group acting: Policy::sample of the selected members in ONE launch of k_candle_act_group (candle_act_group.hpp) -----------------
// group_act.hpp's call with CandleActKind (candle_act_group.hpp), the acting kind of every CandleAgent member: the static half keyed on
// the actor arena, the member's mode and noise counter per call.
using IqlActKind = CandleActKind<Iql>;

// ---- what is IQL's of the group core (group_core.hpp) ----------------------------------------------------------------------------------
struct IqlGroupKind {
    using Member = Iql; using Shape = IgShape; using Launch = IgLaunch; using Step = IqlStep; using MemberArgs = IqlMemberArgs; using PlanMember = IgMember;
    using Act = IqlActKind;
    static constexpr const char *KIND = "iql", *A = "an IQL", *NAME = "IQL", *CAP_MSG = "cap_per_member must hold the three keys of an IQL record";
    static constexpr int MAX_LAUNCHES = IG_MAX_LAUNCHES, K_GATHER = IG_K_GATHER, FORM = BDR_GROUP_FORM_IQL_LAYERS, MIN_CAP = Iql::N_RECORD;
    static IgMember describe(const Iql* m) { return IgMember{iql_shape(m), 1, m->cfg.n_updates_per_opt, m->device, m->prof ? 1 : 0, m->grad_comm ? 1 : 0, m}; }
    static int refusal(const IgMember* m, unsigned n, const char** why, int* kernel) { return ig_group_refusal(m, n, why, kernel); }
    static const char* kernel_name(int k) { return ig_kernel_name(k); }
    static int round_plan(const IgShape& s, unsigned P, IgLaunch* out) { return ig_round_plan(s, P, out); }
    static int launch_count(const IgShape& s) { return ig_launch_count(s.value.n_layers, s.critic.n_layers, s.actor.n_layers); }
    // CandleAgent::opt / Iql::update on the host, in their order
    static IqlStep fill_step(Iql* m, int bs, const GatherArgs& plan)
    {
        IqlStep st{};
        st.word_pos = plan.word_pos; st.size = plan.size;
        m->step_v += 1;
        st.adam[IG_NET_VALUE] = DenseAgent::opt_scalars(m->cfg.opt_value, m->cfg.lr_value, m->step_v);
        m->step_q += 1;
        st.adam[IG_NET_CRITIC] = DenseAgent::opt_scalars(m->cfg.opt_critic, m->cfg.lr_critic, m->step_q);
        m->step_pi += 1;
        st.adam[IG_NET_ACTOR] = DenseAgent::opt_scalars(m->cfg.opt_actor, m->cfg.lr_actor, m->step_pi);
        m->n_opts += 1;
        m->last_B = bs;
        return st;
    }
    static void member_static(Iql* m, int bs, const bdr_replay* r, const GatherArgs& plan, IqlMemberArgs& o) { iql_member_static(m, bs, r, plan, o); }

    int ndense = 0;   // forward and dX launches of a round
    StagedArray<GatherArgs> gather; StagedArray<IqlPackArgs> pack; StagedArray<IqlValueArgs> vloss; StagedArray<IqlCriticArgs> closs; StagedArray<IqlActorArgs> aloss;
    StagedArray<DenseGroupEntry> dense;                                   // [ndense][P] (launch order)
    StagedArray<DenseDwSmallGroup> dw; StagedArray<ReduceAdamArgs> ra;   // [3][P] by IgNetId
    hipError_t allocate(const IgShape& s, size_t P)
    {
        ndense = ig_dense_launches(s.value.n_layers, s.critic.n_layers, s.actor.n_layers);
        hipError_t e = staged_resize(P, gather, pack);   // (in this order: where the arrays lie in device memory shows in the round time, LAB.md)
        if (e == hipSuccess) e = dense.resize((size_t)ndense * P);
        if (e == hipSuccess) e = staged_resize(P, vloss, closs, aloss);
        return e == hipSuccess ? staged_resize(3 * P, dw, ra) : e;
    }
    // member p's arguments into the staging arrays
    void stage(size_t p, size_t P, const IqlMemberArgs& o)
    {
        gather[p] = o.gather; pack[p] = o.pack; vloss[p] = o.vloss; closs[p] = o.closs; aloss[p] = o.aloss;
        for (int i = 0; i < ndense; ++i) dense[(size_t)i * P + p] = o.dense[i];
        for (int n = 0; n < 3; ++n) { dw[(size_t)n * P + p] = o.dw[n]; ra[(size_t)n * P + p] = o.ra[n]; }
    }
    hipError_t upload() { return staged_upload(gather, pack, dense, vloss, closs, aloss, dw, ra); }
    int32_t check_static(const IgLaunch* plan, int n_launches, const IqlMemberArgs& o, uint32_t p) const
    {
        BDR_REQUIRE((int)o.dense.size() == ndense, "member %u: %d dense launches, the plan has %d", p, (int)o.dense.size(), ndense);
        for (int n = 0; n < n_launches; ++n)
            if (plan[n].kernel == IG_K_DW) {
                const int id = plan[n].net;
                BDR_REQUIRE(o.dw_grid[id] == (int)plan[n].gx, "member %u: the weight-gradient grid of network %d (%d) differs from the plan's (%u)", p, id, o.dw_grid[id],
                            plan[n].gx);
            }
        return BDR_OK;
    }
    // one round's launches on the group's stream, grids from the plan; the last one publishes `seq_no`
    int32_t launch(const GroupCore<IqlGroupKind>& g, size_t P, const IqlStep* steps_dev, unsigned seq_no) const
    {
        int nd = 0;
        hipStream_t stream = g.stream;
        for (int n = 0; n < g.n_launches; ++n) {
            const IgLaunch& l = g.plan[n];
            const dim3 grid(l.gx, l.gy, l.gz), block(l.threads);
            const auto* st = (const BDR_CONST_AS IqlStep*)steps_dev;
            switch (l.kernel) {
            case IG_K_GATHER:
                BDR_TRY(replay_gather_group(stream, gather.d.get(), steps_dev, (uint32_t)sizeof(IqlStep), (uint32_t)P, (uint64_t)g.shape.batch, (uint64_t)g.shape.obs_dim * 4));
                break;
            case IG_K_PACK: hipLaunchKernelGGL(k_iql_pack_group, grid, block, 0, stream, (const BDR_CONST_AS IqlPackArgs*)pack.d.get()); break;
            case IG_K_FWD:
                BDR_REQUIRE(nd < ndense, "IQL group round: more dense launches in the plan than argument entries");
                hipLaunchKernelGGL(k_dense_small_members_z<false>, grid, block, 0, stream, (const BDR_CONST_AS DenseGroupEntry*)(dense.d.get() + (size_t)nd++ * P));
                break;
            case IG_K_DX:
                BDR_REQUIRE(nd < ndense, "IQL group round: more dense launches in the plan than argument entries");
                hipLaunchKernelGGL(k_dense_small_members_z<true>, grid, block, 0, stream, (const BDR_CONST_AS DenseGroupEntry*)(dense.d.get() + (size_t)nd++ * P));
                break;
            case IG_K_VALUE_LOSS: hipLaunchKernelGGL(k_iql_value_loss_group, grid, block, 0, stream, (const BDR_CONST_AS IqlValueArgs*)vloss.d.get()); break;
            case IG_K_CRITIC_LOSS: hipLaunchKernelGGL(k_iql_critic_loss_group, grid, block, 0, stream, (const BDR_CONST_AS IqlCriticArgs*)closs.d.get()); break;
            case IG_K_ACTOR_LOSS: hipLaunchKernelGGL(k_iql_actor_loss_group, grid, block, 0, stream, (const BDR_CONST_AS IqlActorArgs*)aloss.d.get()); break;
            case IG_K_DW:
                BDR_REQUIRE(l.net >= 0 && l.net < 3, "IQL group round: launch %d of the plan names no network", n);
                hipLaunchKernelGGL(k_dense_dw_small_members, grid, block, 0, stream, (const BDR_CONST_AS DenseDwSmallGroup*)(dw.d.get() + (size_t)l.net * P));
                break;
            case IG_K_REDUCE_ADAM: {
                BDR_REQUIRE(l.net >= 0 && l.net < 3, "IQL group round: launch %d of the plan names no network", n);
                const auto* a = (const BDR_CONST_AS ReduceAdamArgs*)(ra.d.get() + (size_t)l.net * P);
                if (l.net == IG_NET_VALUE) hipLaunchKernelGGL(k_iql_reduce_adam_group<IG_NET_VALUE>, grid, block, 0, stream, a, st, g.ticket.get(), g.seq.dev, seq_no);
                else if (l.net == IG_NET_CRITIC) hipLaunchKernelGGL(k_iql_reduce_adam_group<IG_NET_CRITIC>, grid, block, 0, stream, a, st, g.ticket.get(), g.seq.dev, seq_no);
                else hipLaunchKernelGGL(k_iql_reduce_adam_group<IG_NET_ACTOR>, grid, block, 0, stream, a, st, g.ticket.get(), g.seq.dev, seq_no);
                break;
            }
            default: return fail(BDR_ERR_INVALID, "IQL group round: launch %d of the plan names no kernel", n);
            }
            BDR_HIP(hipGetLastError());
        }
        return BDR_OK;
    }
};

}  // namespace

struct bdr_iql_group : GroupCore<IqlGroupKind> {};

namespace bdr {
int iql_group_act_dim(const void* group, uint32_t member) { return group_act_dim<bdr_iql_group>(group, member); }   // (trainer.hip)
}  // namespace bdr

extern "C" {

int32_t bdr_iql_group_create(bdr_agent* const* agents, uint32_t n, bdr_iql_group** out) { return group_create(agents, n, out); }
int32_t bdr_iql_group_destroy(bdr_iql_group* g) { return group_destroy(g); }
int32_t bdr_iql_group_size(const bdr_iql_group* g, uint32_t* n) { return group_size(g, n); }
int32_t bdr_iql_group_member(const bdr_iql_group* g, uint32_t i, bdr_agent** out) { return group_member(g, i, out); }
int32_t bdr_iql_group_info(const bdr_iql_group* g, bdr_group_info* out) { return group_info(g, out); }
int32_t bdr_iql_group_opt(bdr_iql_group* g, bdr_replay* const* buffers) { return group_opt(g, buffers); }
int32_t bdr_iql_group_opt_with_scalars(bdr_iql_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    return group_opt_with_scalars(g, buffers, out, cap_per_member, n_out);
}
int32_t bdr_iql_group_sample(bdr_iql_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    return group_sample(g, norms, n, rows, dtypes, act_out);
}
int32_t bdr_iql_group_sample_members(bdr_iql_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n,
                                     const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    return group_sample_members(g, members, n_sel, norms, n, rows, dtypes, act_out);
}
int32_t bdr_iql_group_sync(bdr_iql_group* g) { return group_sync(g); }

}  // extern "C"
