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
// sync - is group_core.hpp's, shared with the other groups; the staging of the gather, dense, dW and reduce launches and the walk over
// the plan are dense_group.hpp's, shared with the AWAC and candle SAC groups, which also states the bounds of member, instance and the
// shared argument arrays.  IqlGroupKind below says what is IQL's.  Per step a member has an IqlStep: the gather reads word_pos and size
// (GatherStepWords at its start), the three reduce + Adam launches its three AdamScalars (value 0, critic 1, actor 2).  The CRITICS
// track their targets; the ACTOR's reduce + Adam is the LAST launch of a round that reads the slot, so it alone publishes.
// Bounds of IQL's own indices: member = blockIdx.y < gridDim.y = P = the length of pack, vloss, closs and aloss; inside a member every
// index is the body's own, with the bounds of the standalone kernel.
// Acting: Policy::sample of the selected members in ONE launch of k_candle_act_group (candle_act_group.hpp, which states the bounds of
// its indices) through group_act.hpp, the host half BC's group shares; IqlActKind below is CandleActKind of an Iql.
#pragma once
#include "dense_group.hpp"
#include "candle_act_group.hpp"
#include "group_core.hpp"
#include "iql_group_plan.hpp"

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
// reduce + Adam of network NET of every member (dense_group.hpp): the critics track their targets, the actor's is the last reader of
// the slot and publishes
template <int NET>
__global__ __launch_bounds__(256) void k_iql_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS IqlStep* steps, unsigned* ticket,
                                                               unsigned* seq_host, unsigned seq)
{
    dg_reduce_adam_step<NET, NET == IG_NET_CRITIC, NET == IG_NET_ACTOR>(args, steps, ticket, seq_host, seq);
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
struct IqlMemberArgs : DenseMemberArgs<3> {   // (dw, dw_grid, ra by IgNetId)
    IqlPackArgs pack; IqlValueArgs vloss; IqlCriticArgs closs; IqlActorArgs aloss;
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
    o.gather = dg_gather_static(r, plan);
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
struct IqlGroupKind : DenseRound<3, IG_K_DW, IG_K_REDUCE_ADAM> {
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

    static constexpr DgReduceEntry<IqlStep> RA[] = {k_iql_reduce_adam_group<IG_NET_VALUE>, k_iql_reduce_adam_group<IG_NET_CRITIC>, k_iql_reduce_adam_group<IG_NET_ACTOR>};
    StagedArray<IqlPackArgs> pack; StagedArray<IqlValueArgs> vloss; StagedArray<IqlCriticArgs> closs; StagedArray<IqlActorArgs> aloss;   // [P]
    hipError_t allocate(const IgShape& s, size_t P)
    {
        return allocate_round(ig_dense_launches(s.value.n_layers, s.critic.n_layers, s.actor.n_layers), P, pack, [&] { return staged_resize(P, vloss, closs, aloss); });
    }
    // member p's arguments into the staging arrays
    void stage(size_t p, size_t P, const IqlMemberArgs& o)
    {
        stage_dense(p, P, o);
        pack[p] = o.pack; vloss[p] = o.vloss; closs[p] = o.closs; aloss[p] = o.aloss;
    }
    hipError_t upload() { return staged_upload(gather, pack, dense, vloss, closs, aloss, dw, ra); }
    int32_t launch(const GroupCore<IqlGroupKind>& g, size_t P, const IqlStep* steps_dev, unsigned seq_no) const { return dg_round_launch(g, P, steps_dev, seq_no, *this); }
    // IQL's own launches of a round
    int32_t launch_own(const IgLaunch& l, int n, size_t, dim3 grid, dim3 block, const BDR_CONST_AS IqlStep*, hipStream_t stream) const
    {
        switch (l.kernel) {
        case IG_K_PACK: hipLaunchKernelGGL(k_iql_pack_group, grid, block, 0, stream, (const BDR_CONST_AS IqlPackArgs*)pack.d.get()); break;
        case IG_K_VALUE_LOSS: hipLaunchKernelGGL(k_iql_value_loss_group, grid, block, 0, stream, (const BDR_CONST_AS IqlValueArgs*)vloss.d.get()); break;
        case IG_K_CRITIC_LOSS: hipLaunchKernelGGL(k_iql_critic_loss_group, grid, block, 0, stream, (const BDR_CONST_AS IqlCriticArgs*)closs.d.get()); break;
        case IG_K_ACTOR_LOSS: hipLaunchKernelGGL(k_iql_actor_loss_group, grid, block, 0, stream, (const BDR_CONST_AS IqlActorArgs*)aloss.d.get()); break;
        default: return fail(BDR_ERR_INVALID, "IQL group round: launch %d of the plan names no kernel", n);
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
int32_t bdr_iql_group_copy_members(bdr_iql_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags)
{
    return group_copy_members(g, src, dst, n, flags);
}

}  // extern "C"
