// ================================================================================================
// A group of AWAC agents: Awac::opt_ (awac/base.rs:170-215) of every member in the launch sequence Awac::update enqueues for ONE member -
// gather, pack, the actor on obs, the sample of act_, the online critics on (obs | act) and (obs | act_), the actor loss and the actor's
// step, the updated actor on next_obs, the sample of next_act, the target critics on (next_obs | next_act), the critic loss and the
// critics' step with the soft update riding on it - with every launch serving ALL members: the member index is grid dimension y, the
// network instance (where the standalone launch has one) stays grid dimension z, x stays the member's own grid (awac_group_plan.hpp
// has the rule and the grids).  A launch grouping, not an agent kind: the members stay ordinary AWAC agents on the group's stream.  A
// part of awac.hip's translation unit (it needs Awac and the bodies of AWAC's kernels), included where the code stands.
// Each entry runs the body of the kernel it groups (awac.hip, candle_actor.hpp, dense.hpp, replay.hip) on the member's entry of a device
// array, read in place through the constant address space: member and instance come from blockIdx, so they are uniform and the entry's
// fields are scalar loads, as they are from the kernel-argument segment of the standalone kernel.  Same bodies, same bits.  The actor
// loss keeps its A + 1 workgroups per member, the critic loss its one: candle::row_sum / row_max run inside a workgroup, in their block
// order, over the member's rows only.
// The host half - the members' adoption, the static argument arrays and their keys, the step ring and its slot rule, the round, records,
// sync - is group_core.hpp's, shared with the other groups; the staging of the gather, dense, dW and reduce launches and the walk over
// the plan are dense_group.hpp's, shared with the IQL and candle SAC groups, which also states the bounds of member, instance and the
// shared argument arrays.  AwacGroupKind below says what is AWAC's.  Per step a member has an AwacStep: the gather reads word_pos and
// size (GatherStepWords at its start), the two reduce + Adam launches its two AdamScalars (actor 0, critic 1), the two sample launches
// its mode and their counter.  The CRITICS track their targets, and their reduce + Adam is the LAST launch of a round that reads the
// slot, so it alone publishes.
// The noise rule.  AWAC draws inside the round: act_ = actor.sample(obs) and next_act = actor.sample(next_obs).  fill_step does per
// member what CandleAgent::opt and Awac::update do on the host, in their order: it reads the member's mode NOW, and in train mode takes
// B A draws of the member's noise_counter for act_, then B A for next_act (sample_elem's rule; eval mode takes none), then advances
// step_pi, step_q, n_opts and last_B.  Element t of a sample launch draws at its counter + t, as in k_candle_sample.  The counter is
// the one the member's own sample / update_on_batch / bdr_agent_draw_noise and the group's acting calls advance: one stream in any
// interleaving, and bdr_agent_set_train on a member between rounds takes effect in the next round without restaging.
// Bounds of AWAC's own indices:
//   member = blockIdx.y < gridDim.y = P = the length of pack, aloss and closs;
//   the sample launch of draw d (act_ 0, next_act 1) is handed sample + d * P: 2 P entries; d < 2 = the counters of an AwacStep; its
//   t = blockIdx.x * 256 + threadIdx.x is used only where t < n A = B A, the elements of the member's out block ([B][A]) and of the
//   action columns O .. O + A of its critic input ([B][ldq], O + A <= ldq); the draw index counter + t is a 64-bit sum;
//   the actor loss has gridDim.x = A + 1: workgroup j < A writes column j of gmean ([B][ldm], A <= ldm) and gh2[j];
//   inside a member every other index is the body's own, with the bounds of the standalone kernel.
// Memory traffic is plain vector stores, the existing agent-scope atomics of the ticket and st_agent / ld_agent: nothing new.
// Acting: Policy::sample of the selected members in ONE launch of k_candle_act_group (candle_act_group.hpp, which states the bounds of
// its indices) through group_act.hpp; AwacActKind below is CandleActKind of an Awac.
// Online: bdr_awac_group_push is group_core.hpp's group_push (n transitions per member into the member's own ring, ONE launch of
// k_cgroup_push, group_push.hpp); the compiled online loop over the group is bdr_trainer_train_cgroup_post (trainer.hip).
#pragma once
#include "dense_group.hpp"
#include "candle_act_group.hpp"
#include "group_core.hpp"
#include "awac_group_plan.hpp"

// the per-step words of one member: the gather's, then the optimizer scalars of actor and critics (AgNetId's order), the mode, and the
// noise counters of the act_ and the next_act launch
struct AwacStep { unsigned long long word_pos, size; AdamScalars adam[2]; int train; unsigned long long counter[2]; };
static_assert(offsetof(AwacStep, word_pos) == offsetof(GatherStepWords, word_pos) && offsetof(AwacStep, size) == offsetof(GatherStepWords, size),
              "the grouped gather reads the first two words of a member's AwacStep");
static_assert(AG_NET_ACTOR == 0 && AG_NET_CRITIC == 1, "AwacStep::adam and the dW / reduce argument arrays are indexed by AgNetId");

namespace {

// ---- the group entries: grid dimension y is the member -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_awac_pack_group(const BDR_CONST_AS AwacPackArgs* args) { awac_pack_body(args[blockIdx.y]); }
__global__ __launch_bounds__(1024) void k_awac_actor_loss_group(const BDR_CONST_AS AwacActorArgs* args)
{
    __shared__ float red[32];
    awac_actor_loss_body(args[blockIdx.y], red);
}
__global__ __launch_bounds__(1024) void k_awac_critic_loss_group(const BDR_CONST_AS AwacCriticArgs* args)
{
    __shared__ float red[32];
    awac_critic_loss_body(args[blockIdx.y], red);
}
// Policy::sample of every member's B rows, draw `d` of the round (0: act_, 1: next_act): the static half of the element code's operands
// (head2, the clamps, the limit, the seed, mlp2 = 0) from the member's entry, the mode and the counter from its step slot, z null
__global__ __launch_bounds__(256) void k_awac_sample_group(const BDR_CONST_AS CandleSampleArgs* args, const BDR_CONST_AS AwacStep* steps, int d)
{
    const BDR_CONST_AS CandleSampleArgs& a = args[blockIdx.y];
    const BDR_CONST_AS AwacStep& st = steps[blockIdx.y];
    SampleElem e;   // field by field: static indices, registers
    e.head2 = a.e.head2; e.lo = a.e.lo; e.hi = a.e.hi; e.tanh_limit = a.e.tanh_limit; e.amin = a.e.amin; e.amax = a.e.amax; e.scale = a.e.scale;
    e.train = st.train; e.seed = a.e.seed; e.counter = d ? st.counter[1] : st.counter[0]; e.z = nullptr; e.mlp2 = a.e.mlp2;
    candle_sample_body(a, e);
}
// reduce + Adam of network NET of every member (dense_group.hpp): the critics track their targets, are the last reader of the slot
// and publish
template <int NET>
__global__ __launch_bounds__(256) void k_awac_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS AwacStep* steps, unsigned* ticket,
                                                                unsigned* seq_host, unsigned seq)
{
    dg_reduce_adam_step<NET, NET == AG_NET_CRITIC, NET == AG_NET_CRITIC>(args, steps, ticket, seq_host, seq);
}

AgShape awac_shape(const Awac* m)
{
    AgShape s{};
    s.obs_dim = m->O; s.act_dim = m->A; s.batch = (int)m->cfg.batch_size; s.n_critics = m->NC;
    s.critic = dg_net_shape(m->qn, m->cfg.critic.activation_out);
    s.actor = dg_net_shape(m->pn, m->cfg.actor.activation_out);
    return s;
}

// ---- host: one member's static arguments, exactly what Awac::update hands its launches --------------------------------------------------
struct AwacMemberArgs : DenseMemberArgs<2> {   // (dw, dw_grid, ra by AgNetId)
    AwacPackArgs pack;
    CandleSampleArgs sample[2];           // act_, next_act (train, counter and z are the step's)
    AwacActorArgs aloss; AwacCriticArgs closs;
};

// (bs: the batch size; r: the member's ring or view; plan: replay_sample_plan's descriptor of this step)
void awac_member_static(Awac* m, int bs, const bdr_replay* r, const GatherArgs& plan, AwacMemberArgs& o)
{
    const bdr_awac_config& cfg = m->cfg;
    const int NC = m->NC, O = m->O, A = m->A;
    const MlpLayout &qn = m->qn, &pn = m->pn;
    const int Lq = (int)qn.L.size(), Lp = (int)pn.L.size();
    const int ldq = qn.L[Lq - 1].Np;
    const float* obs = reinterpret_cast<const float*>(r->b_obs);
    const float* next_obs = reinterpret_cast<const float*>(r->b_next);
    const float* act = reinterpret_cast<const float*>(r->b_act);
    o.dense.clear();
    o.gather = dg_gather_static(r, plan);
    o.pack = AwacPackArgs{obs, next_obs, act, O, A, bs, m->x_o, m->x_no, pn.L[0].Kp, m->xq, m->xq_pi, m->xq_next, qn.L[0].Kp};
    // CandleAgent::sample_pack with the static half of sample_elem (no host draws under a group: z null)
    const auto sample = [&](const float* mean, float* out, float* xqd) {
        CandleSampleArgs p{};
        p.mean = mean; p.ldm = pn.L.back().Np; p.A = A; p.n = bs;
        SampleElem& e = p.e;
        e.head2 = m->pi_p + m->h2_off; e.mlp2 = 0;
        e.lo = (float)cfg.min_log_std; e.hi = (float)cfg.max_log_std; e.tanh_limit = cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
        e.amin = (float)cfg.action_min; e.amax = (float)cfg.action_max; e.scale = (float)cfg.action_scale;
        e.seed = cfg.seed;
        p.out = out; p.xq = xqd; p.ldq = qn.L[0].Kp; p.O = O;
        return p;
    };
    // ---- update_actor
    { const float* pp[1] = {m->pi_p}; const float* x[1] = {m->x_o}; std::vector<float*>* acts[1] = {&m->p_act}; dg_fwd_entries(o.dense, pn, 1, pp, x, acts, bs); }
    o.sample[0] = sample(m->p_act[Lp - 1], m->pr_act, m->xq_pi);
    {   // the online critics on (obs | act) and (obs | act_): one forward of 2 NC networks
        const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
        for (int i = 0; i < NC; ++i) { params[i] = m->q_p[i]; x[i] = m->xq; acts[i] = &m->c_act[i]; params[NC + i] = m->q_p[i]; x[NC + i] = m->xq_pi; acts[NC + i] = &m->cp_act[i]; }
        dg_fwd_entries(o.dense, qn, 2 * NC, params, x, acts, bs);
    }
    {
        AwacActorArgs& p = o.aloss;
        p = AwacActorArgs{};
        for (int i = 0; i < NC; ++i) { p.qd[i] = m->c_act[i][Lq - 1]; p.qp[i] = m->cp_act[i][Lq - 1]; }
        p.ldq = ldq; p.NC = NC;
        p.mean = m->p_act[Lp - 1]; p.ldm = pn.L[Lp - 1].Np; p.head2 = m->pi_p + m->h2_off; p.act = act; p.A = A;
        p.lo = (float)cfg.min_log_std; p.hi = (float)cfg.max_log_std; p.tanh_limit = cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
        p.scale = (float)cfg.action_scale; p.inv_lambda = (float)cfg.inv_lambda; p.exp_adv_max = (float)cfg.exp_adv_max; p.softmax = cfg.adv_softmax ? 1 : 0;
        p.q_data = m->pr_qd; p.q_pi = m->pr_qp; p.adv = m->pr_adv; p.w = m->pr_w; p.logp = m->pr_logp; p.gmean = m->p_dy[Lp - 1]; p.gh2 = m->h2_part;
        p.scal = m->scal; p.accumulate = 0; p.B = bs;
    }
    {
        std::vector<float*>* acts[1] = {&m->p_act}; std::vector<float*>* dys[1] = {&m->p_dy};
        const DenseReduceSeg h2seg{m->h2_part, (size_t)pad64(A), 1, (unsigned)(m->h2_off / 4), (unsigned)(pad64(A) / 4)};
        dg_step_entries(o, AG_NET_ACTOR, pn, 1, &m->pi_p, &m->pi_g, &m->pi_m, &m->pi_v, nullptr, m->x_o, acts, dys, m->pi_part, 0, m->pi_off, bs, m->pi_total,
                        cfg.critic_tau, &h2seg);
    }
    // ---- update_critic
    { const float* pp[1] = {m->pi_p}; const float* x[1] = {m->x_no}; std::vector<float*>* acts[1] = {&m->pn_act}; dg_fwd_entries(o.dense, pn, 1, pp, x, acts, bs); }
    o.sample[1] = sample(m->pn_act[Lp - 1], m->pr_next_act, m->xq_next);
    {
        const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
        for (int i = 0; i < NC; ++i) { params[i] = m->q_t[i]; x[i] = m->xq_next; acts[i] = &m->t_act[i]; }
        dg_fwd_entries(o.dense, qn, NC, params, x, acts, bs);
    }
    {
        AwacCriticArgs& p = o.closs;
        p = AwacCriticArgs{};
        for (int i = 0; i < NC; ++i) { p.q[i] = m->c_act[i][Lq - 1]; p.dq[i] = m->c_dy[i][Lq - 1]; p.qt[i] = m->t_act[i][Lq - 1]; }
        p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu;
        p.reward = r->b_reward; p.term = r->b_term; p.trunc = r->b_trunc; p.gamma = (float)cfg.gamma; p.tgt = m->pr_tgt; p.next_q = m->pr_nq;
        p.loss_kind = cfg.critic_loss; p.scal = m->scal; p.accumulate = 0; p.B = bs;
    }
    {
        std::vector<float*>* acts[4]; std::vector<float*>* dys[4];
        for (int i = 0; i < NC; ++i) { acts[i] = &m->c_act[i]; dys[i] = &m->c_dy[i]; }
        dg_step_entries(o, AG_NET_CRITIC, qn, NC, m->q_p, m->q_g, m->q_m, m->q_v, m->q_t, m->xq, acts, dys, m->q_part, m->q_part_stride, m->q_off, bs, qn.total,
                        cfg.critic_tau, nullptr);
    }
}

using AwacActKind = CandleActKind<Awac>;   // group acting (candle_act_group.hpp)

// ---- what is AWAC's of the group core (group_core.hpp) ---------------------------------------------------------------------------------
struct AwacGroupKind : DenseRound<2, AG_K_DW, AG_K_REDUCE_ADAM> {
    using Member = Awac; using Shape = AgShape; using Launch = AgLaunch; using Step = AwacStep; using MemberArgs = AwacMemberArgs; using PlanMember = AgMember;
    using Act = AwacActKind;
    static constexpr const char *KIND = "awac", *A = "an AWAC", *NAME = "AWAC", *CAP_MSG = "cap_per_member must hold the eight keys of an AWAC record";
    static constexpr int MAX_LAUNCHES = AG_MAX_LAUNCHES, K_GATHER = AG_K_GATHER, FORM = BDR_GROUP_FORM_AWAC_LAYERS, MIN_CAP = Awac::N_RECORD;
    static AgMember describe(const Awac* m) { return AgMember{awac_shape(m), 1, m->cfg.n_updates_per_opt, m->device, m->prof ? 1 : 0, m->grad_comm ? 1 : 0, m}; }
    static int refusal(const AgMember* m, unsigned n, const char** why, int* kernel) { return ag_group_refusal(m, n, why, kernel); }
    static const char* kernel_name(int k) { return ag_kernel_name(k); }
    static int round_plan(const AgShape& s, unsigned P, AgLaunch* out) { return ag_round_plan(s, P, out); }
    static int launch_count(const AgShape& s) { return ag_launch_count(s.critic.n_layers, s.actor.n_layers); }
    // CandleAgent::opt / Awac::update on the host, in their order: the mode now, the draws of act_ and next_act (sample_elem), the
    // actor's step, the critics' step, n_opts, last_B
    static AwacStep fill_step(Awac* m, int bs, const GatherArgs& plan)
    {
        AwacStep st{};
        st.word_pos = plan.word_pos; st.size = plan.size;
        st.train = m->train ? 1 : 0;
        if (st.train)
            for (int d = 0; d < 2; ++d) { st.counter[d] = m->noise_counter; m->noise_counter += (uint64_t)bs * m->A; }
        m->step_pi += 1;
        st.adam[AG_NET_ACTOR] = DenseAgent::opt_scalars(m->cfg.opt_actor, m->cfg.lr_actor, m->step_pi);
        m->step_q += 1;
        st.adam[AG_NET_CRITIC] = DenseAgent::opt_scalars(m->cfg.opt_critic, m->cfg.lr_critic, m->step_q);
        m->n_opts += 1;
        m->last_B = bs;
        return st;
    }
    static void member_static(Awac* m, int bs, const bdr_replay* r, const GatherArgs& plan, AwacMemberArgs& o) { awac_member_static(m, bs, r, plan, o); }

    static constexpr DgReduceEntry<AwacStep> RA[] = {k_awac_reduce_adam_group<AG_NET_ACTOR>, k_awac_reduce_adam_group<AG_NET_CRITIC>};
    StagedArray<AwacPackArgs> pack; StagedArray<AwacActorArgs> aloss; StagedArray<AwacCriticArgs> closs;   // [P]
    StagedArray<CandleSampleArgs> sample;                                                                  // [2][P]: act_, next_act
    hipError_t allocate(const AgShape& s, size_t P)
    {
        return allocate_round(ag_dense_launches(s.critic.n_layers, s.actor.n_layers), P, pack, [&] {
            const hipError_t e = staged_resize(P, aloss, closs);
            return e == hipSuccess ? sample.resize(2 * P) : e;
        });
    }
    // member p's arguments into the staging arrays
    void stage(size_t p, size_t P, const AwacMemberArgs& o)
    {
        stage_dense(p, P, o);
        pack[p] = o.pack; aloss[p] = o.aloss; closs[p] = o.closs;
        for (int d = 0; d < 2; ++d) sample[(size_t)d * P + p] = o.sample[d];
    }
    hipError_t upload() { return staged_upload(gather, pack, dense, sample, aloss, closs, dw, ra); }
    int32_t launch(const GroupCore<AwacGroupKind>& g, size_t P, const AwacStep* steps_dev, unsigned seq_no) const { return dg_round_launch(g, P, steps_dev, seq_no, *this); }
    // AWAC's own launches of a round
    int32_t launch_own(const AgLaunch& l, int n, size_t P, dim3 grid, dim3 block, const BDR_CONST_AS AwacStep* st, hipStream_t stream) const
    {
        switch (l.kernel) {
        case AG_K_PACK: hipLaunchKernelGGL(k_awac_pack_group, grid, block, 0, stream, (const BDR_CONST_AS AwacPackArgs*)pack.d.get()); break;
        case AG_K_SAMPLE:
            BDR_REQUIRE(l.layer == 0 || l.layer == 1, "AWAC group round: launch %d of the plan names no draw", n);
            hipLaunchKernelGGL(k_awac_sample_group, grid, block, 0, stream, (const BDR_CONST_AS CandleSampleArgs*)(sample.d.get() + (size_t)l.layer * P), st, l.layer);
            break;
        case AG_K_ACTOR_LOSS: hipLaunchKernelGGL(k_awac_actor_loss_group, grid, block, 0, stream, (const BDR_CONST_AS AwacActorArgs*)aloss.d.get()); break;
        case AG_K_CRITIC_LOSS: hipLaunchKernelGGL(k_awac_critic_loss_group, grid, block, 0, stream, (const BDR_CONST_AS AwacCriticArgs*)closs.d.get()); break;
        default: return fail(BDR_ERR_INVALID, "AWAC group round: launch %d of the plan names no kernel", n);
        }
        return BDR_OK;
    }
};

}  // namespace

struct bdr_awac_group : GroupCore<AwacGroupKind> {};

namespace bdr {
int awac_group_act_dim(const void* group, uint32_t member) { return group_act_dim<bdr_awac_group>(group, member); }   // (trainer.hip)
int awac_group_obs_dim(const void* group, uint32_t member) { return group_obs_dim<bdr_awac_group>(group, member); }   // (trainer.hip)
}  // namespace bdr

extern "C" {

int32_t bdr_awac_group_create(bdr_agent* const* agents, uint32_t n, bdr_awac_group** out) { return group_create(agents, n, out); }
int32_t bdr_awac_group_destroy(bdr_awac_group* g) { return group_destroy(g); }
int32_t bdr_awac_group_size(const bdr_awac_group* g, uint32_t* n) { return group_size(g, n); }
int32_t bdr_awac_group_member(const bdr_awac_group* g, uint32_t i, bdr_agent** out) { return group_member(g, i, out); }
int32_t bdr_awac_group_info(const bdr_awac_group* g, bdr_group_info* out) { return group_info(g, out); }
int32_t bdr_awac_group_opt(bdr_awac_group* g, bdr_replay* const* buffers) { return group_opt(g, buffers); }
int32_t bdr_awac_group_opt_with_scalars(bdr_awac_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    return group_opt_with_scalars(g, buffers, out, cap_per_member, n_out);
}
int32_t bdr_awac_group_sample(bdr_awac_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    return group_sample(g, norms, n, rows, dtypes, act_out);
}
int32_t bdr_awac_group_sample_members(bdr_awac_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n,
                                      const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    return group_sample_members(g, members, n_sel, norms, n, rows, dtypes, act_out);
}
int32_t bdr_awac_group_sync(bdr_awac_group* g) { return group_sync(g); }
int32_t bdr_awac_group_copy_members(bdr_awac_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags)
{
    return group_copy_members(g, src, dst, n, flags);
}
int32_t bdr_awac_group_push(bdr_awac_group* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs, const void* const* next_obs, const int32_t* obs_dtypes,
        const float* const* act, const float* const* reward, const int8_t* const* is_terminated, const int8_t* const* is_truncated)
{
    return group_push(g, buffers, n, obs, next_obs, obs_dtypes, act, reward, is_terminated, is_truncated);
}
int32_t bdr_awac_group_push_max_rows(bdr_awac_group* g, bdr_replay* const* buffers, const int32_t* obs_dtypes, uint64_t* n_max)
{
    return group_push_max_rows(g, buffers, obs_dtypes, n_max);
}

}  // extern "C"
