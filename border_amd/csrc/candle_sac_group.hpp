// ================================================================================================
// A group of candle SAC agents: Sac::opt_ (sac/base.rs:124-134) of every member in the launch sequence CandleSac::update enqueues for
// ONE member behind the gather - pack, the actor on obs, sample + logp of a with its partials, the entropy coefficient's step, the
// online critics on (obs | act) and (obs | a), qmin, the critics' input-gradient chain down to d(-q/B)/da, the actor's output gradient
// and its step, the updated actor on next_obs, sample + logp of next_a, the target critics on (next_obs | next_a), the critic loss and
// the critics' step with the soft update riding on it - with every launch serving ALL members: the member index is grid dimension y,
// the network instance (where the standalone launch has one) stays grid dimension z, x stays the member's own grid
// (candle_sac_group_plan.hpp has the rule and the grids).  A launch grouping, not an agent kind: the members stay ordinary candle SAC
// agents on the group's stream.  A part of candle_sac.hip's translation unit (it needs CandleSac and the bodies of SAC's kernels),
// included where the code stands.
// Each entry runs the body of the kernel it groups (candle_sac.hip, dense.hpp, replay.hip) on the member's entry of a device array,
// read in place through the constant address space: member and instance come from blockIdx, so they are uniform and the entry's
// fields are scalar loads, as they are from the kernel-argument segment of the standalone kernel.  Same bodies, same bits.  The actor
// gradient keeps its A + 1 workgroups per member, alpha and the critic loss their one: candle::row_sum runs inside a workgroup, in its
// block order, over the member's rows only; the butterfly of sample + logp stays inside the G lanes of one row of one member.
// The host half - the members' adoption, the static argument arrays and their keys, the step ring and its slot rule, the round,
// records, sync - is group_core.hpp's, shared with the other groups; the staging of the gather, dense, dW and reduce launches and the
// walk over the plan are dense_group.hpp's, shared with the IQL and AWAC groups, which also states the bounds of member, instance and
// the shared argument arrays.  CandleSacGroupKind below says what is SAC's.  Per step a member has a CsacStep: the gather reads
// word_pos and size (GatherStepWords at its start), the two reduce + Adam launches (actor 0, critic 1) and the alpha launch their
// AdamScalars, the two sample + logp launches the mode and their counter.  The CRITICS track their targets, and their reduce + Adam
// is the LAST launch of a round that reads the slot, so it alone publishes.
// What a SAC round adds to the groups before it.  (1) A third optimizer: the entropy coefficient's AdamW step, per member Fix or Auto
// (auto_mode and target_entropy are static words of the member's alpha entry; its AdamScalars are step words, written in Auto mode
// only and read in Auto mode only).  (2) The action gradient: the critics' input-gradient chain runs through k_dense_small_members_z<dx>
// with nz = NC; its input-layer entry has a null mask (dense_small_body reads a.mask per entry and takes 1 where it is null, as
// dense_dx_z's launch does today) and writes into dxa.  (3) Mlp2 actors: the last layer is [mean | s]; mlp2 is a static word of the
// member's sample and actor-gradient entries, head2 / gh2 are not read in that form.  (4) Online members: a member's ring grows and
// wraps between rounds through the grouped push (bdr_candle_sac_group_push: group_core.hpp's group_push, ONE launch for all members)
// or its own rb.push; word_pos and size are step words and the gather's static half is keyed on the ring, so nothing is restaged for
// that.
// The noise rule.  fill_step does per member what CandleAgent::opt and CandleSac::update do on the host, in their order: it reads the
// member's mode NOW, and in train mode takes B A draws of the member's noise_counter for a, then B A for next_a (sample_elem's rule;
// eval mode takes none), then advances step_al (Auto only), step_pi, step_q, n_opts and last_B.  Element t = b A + j of a sample +
// logp launch draws at its counter + t, as in k_csac_sample_logp.  The counter is the one the member's own sample / update_on_batch /
// bdr_agent_draw_noise and the group's acting calls advance: one stream in any interleaving, and bdr_agent_set_train on a member
// between rounds takes effect in the next round without restaging.
// Bounds of SAC's own indices:
//   member = blockIdx.y < gridDim.y = P = the length of pack, alpha, qmin, agrad and closs; the alpha entry reads adam[2] of the three
//   AdamScalars of a CsacStep;
//   the sample + logp launch of draw d (a 0, next_a 1) is handed sample + d * P: 2 P entries; d < 2 = the counters of a CsacStep; its
//   row b = blockIdx.x * (256 / G) + threadIdx.x / G touches memory only where b < B, its column j = g0 + k G only where j < A: the
//   elements of the member's out and g_* blocks ([B][A]), of logp ([B]), of the mean row ([B][ldm], A <= ldm; Mlp2: A + j < 2 A <= ldm)
//   and of the action columns O .. O + A of its critic input ([B][ldq], O + A <= ldq); G = cs_sample_lanes(A) is a power of two
//   <= 64, the same for all members (one act_dim per group), so the grid ceil(B / (256 / G)) covers every member's rows; the draw
//   index counter + t is a 64-bit sum;
//   qmin: b = blockIdx.x * 256 + threadIdx.x is used only where b < B, column 0 of [B][ldq] rows, critic i < NC <= 2;
//   the actor gradient has gridDim.x = A + 1: workgroup j < A reads column O + j of dxa_i ([B][ldx], O + A <= ldx), writes column j
//   (Mlp2: and A + j < 2 A <= ldm) of gout ([B][ldm]), dq_da at b A + j < B A, and (Mlp3) gh2[j], j < A <= pad64(A);
//   alpha: one workgroup, b < B in row_sum, ent holds 8 floats;  critic loss: one workgroup, b < B, column 0 of [B][ldq] rows;
//   inside a member every other index is the body's own, with the bounds of the standalone kernel.
// Memory traffic is plain vector stores, the existing agent-scope atomics of the ticket and st_agent / ld_agent: nothing new.
// Acting: Policy::sample of the selected members in ONE launch of k_candle_act_group (candle_act_group.hpp, which states the bounds of
// its indices, those of an Mlp2 last layer included) through group_act.hpp; CandleSacActKind below is CandleActKind of a CandleSac.
#pragma once
#include "dense_group.hpp"
#include "candle_act_group.hpp"
#include "group_core.hpp"
#include "candle_sac_group_plan.hpp"

static_assert(CS_ACTOR_MLP3 == BDR_ACTOR_MLP3 && CS_ACTOR_MLP2 == BDR_ACTOR_MLP2, "candle_sac_group_plan.hpp restates the actor kinds");

// the per-step words of one member: the gather's, then the optimizer scalars of actor, critics (CsNetId's order) and the entropy
// coefficient, the mode, and the noise counters of the a and the next_a launch
constexpr int CS_ADAM_ALPHA = 2;
struct CsacStep { unsigned long long word_pos, size; AdamScalars adam[3]; int train; unsigned long long counter[2]; };
static_assert(offsetof(CsacStep, word_pos) == offsetof(GatherStepWords, word_pos) && offsetof(CsacStep, size) == offsetof(GatherStepWords, size),
              "the grouped gather reads the first two words of a member's CsacStep");
static_assert(CS_NET_ACTOR == 0 && CS_NET_CRITIC == 1, "CsacStep::adam and the dW / reduce argument arrays are indexed by CsNetId");

namespace {

// ---- the group entries: grid dimension y is the member -------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_csac_pack_group(const BDR_CONST_AS CsacPackArgs* args) { csac_pack_body(args[blockIdx.y]); }
// sample + logp of every member's B rows, draw `d` of the round (0: a, with the partials; 1: next_a, without): the static half (the
// last layer, ldm, head2, mlp2, the clamps, the limit, the seed, the outputs, the gradient outputs or nulls) from the member's entry,
// the mode and the counter from its step slot, z null
__global__ __launch_bounds__(256) void k_csac_sample_logp_group(const BDR_CONST_AS CsacSampleArgs* args, const BDR_CONST_AS CsacStep* steps, int d)
{
    const BDR_CONST_AS CsacStep& st = steps[blockIdx.y];
    csac_sample_logp_body(args[blockIdx.y], st.train, (uint64_t)(d ? st.counter[1] : st.counter[0]), nullptr);
}
// EntCoef::update of every member: logp, B, target_entropy, auto_mode and ent from the member's entry, the AdamW scalars from its slot
__global__ __launch_bounds__(1024) void k_csac_alpha_group(const BDR_CONST_AS CsacAlphaArgs* args, const BDR_CONST_AS CsacStep* steps)
{
    __shared__ float red[32];
    const AdamScalars s = dg_step_scalars(steps[blockIdx.y].adam[CS_ADAM_ALPHA]);
    csac_alpha_body(args[blockIdx.y], s, red);
}
__global__ __launch_bounds__(256) void k_csac_qmin_group(const BDR_CONST_AS CsacQminArgs* args) { csac_qmin_body(args[blockIdx.y]); }
__global__ __launch_bounds__(1024) void k_csac_actor_grad_group(const BDR_CONST_AS CsacActorArgs* args)
{
    __shared__ float red[32];
    csac_actor_grad_body(args[blockIdx.y], red);
}
__global__ __launch_bounds__(1024) void k_csac_critic_loss_group(const BDR_CONST_AS CsacCriticArgs* args)
{
    __shared__ float red[32];
    csac_critic_loss_body(args[blockIdx.y], red);
}
// reduce + Adam of network NET of every member (dense_group.hpp): the critics track their targets, are the last reader of the slot
// and publish
template <int NET>
__global__ __launch_bounds__(256) void k_csac_reduce_adam_group(const BDR_CONST_AS ReduceAdamArgs* args, const BDR_CONST_AS CsacStep* steps, unsigned* ticket,
                                                                unsigned* seq_host, unsigned seq)
{
    dg_reduce_adam_step<NET, NET == CS_NET_CRITIC, NET == CS_NET_CRITIC>(args, steps, ticket, seq_host, seq);
}

CsShape csac_shape(const CandleSac* m)
{
    CsShape s{};
    s.obs_dim = m->O; s.act_dim = m->A; s.batch = (int)m->cfg.batch_size; s.n_critics = m->NC; s.actor_kind = m->actor_kind;
    s.critic = dg_net_shape(m->qn, m->cfg.critic.activation_out);
    s.actor = dg_net_shape(m->pn, m->cfg.actor.activation_out);
    return s;
}

// ---- host: one member's static arguments, exactly what CandleSac::update hands its launches --------------------------------------------
struct CsacMemberArgs : DenseMemberArgs<2> {   // (dw, dw_grid, ra by CsNetId)
    CsacPackArgs pack;
    CsacSampleArgs sample[2];             // a (gradient form), next_a (train, counter and z are the step's)
    CsacAlphaArgs alpha; CsacQminArgs qmin; CsacActorArgs agrad; CsacCriticArgs closs;
};

// (bs: the batch size; r: the member's ring or view; plan: replay_sample_plan's descriptor of this step)
void csac_member_static(CandleSac* m, int bs, const bdr_replay* r, const GatherArgs& plan, CsacMemberArgs& o)
{
    const bdr_candle_sac_config& cfg = m->cfg;
    const int NC = m->NC, O = m->O, A = m->A;
    const MlpLayout &qn = m->qn, &pn = m->pn;
    const int Lq = (int)qn.L.size(), Lp = (int)pn.L.size();
    const int ldq = qn.L[Lq - 1].Np;
    const bool mlp2 = m->mlp2();
    const float* obs = reinterpret_cast<const float*>(r->b_obs);
    const float* next_obs = reinterpret_cast<const float*>(r->b_next);
    const float* act = reinterpret_cast<const float*>(r->b_act);
    o.dense.clear();
    o.gather = dg_gather_static(r, plan);
    o.pack = CsacPackArgs{obs, next_obs, act, O, A, bs, m->x_o, m->x_no, pn.L[0].Kp, m->xq, m->xq_pi, m->xq_next, qn.L[0].Kp};
    // CandleSac::sample_logp with the static half of sample_elem (no host draws under a group: z null)
    const auto sample = [&](const float* last, float* out, float* xqd, float* logp, bool grads) {
        CsacSampleArgs p{};
        p.mean = last; p.ldm = pn.L.back().Np; p.mlp2 = mlp2 ? 1 : 0; p.head2 = mlp2 ? nullptr : m->pi_p + m->h2_off; p.A = A; p.B = bs;
        p.G = cs_sample_lanes(A);
        p.lo = (float)cfg.min_log_std; p.hi = (float)cfg.max_log_std; p.tanh_limit = cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
        p.amin = (float)cfg.action_min; p.amax = (float)cfg.action_max; p.scale = (float)cfg.action_scale;
        p.seed = cfg.seed;
        p.out = out; p.xq = xqd; p.ldq = qn.L[0].Kp; p.O = O; p.logp = logp;
        if (grads) { p.g_lpm = m->g_lpm; p.g_lpl = m->g_lpl; p.g_am = m->g_am; p.g_al = m->g_al; }
        return p;
    };
    // ---- update_actor
    { const float* pp[1] = {m->pi_p}; const float* x[1] = {m->x_o}; std::vector<float*>* acts[1] = {&m->p_act}; dg_fwd_entries(o.dense, pn, 1, pp, x, acts, bs); }
    o.sample[0] = sample(m->p_act[Lp - 1], m->pr_a, m->xq_pi, m->pr_logp, true);
    {
        CsacAlphaArgs& p = o.alpha;
        p = CsacAlphaArgs{};
        p.logp = m->pr_logp; p.B = bs; p.target_entropy = (float)cfg.target_entropy; p.auto_mode = cfg.ent_coef_mode == BDR_ENT_COEF_AUTO ? 1 : 0;
        p.ent = m->ent;   // (s is the step's)
    }
    {   // the online critics on (obs | act) and (obs | a): one forward of 2 NC networks
        const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
        for (int i = 0; i < NC; ++i) { params[i] = m->q_p[i]; x[i] = m->xq; acts[i] = &m->c_act[i]; params[NC + i] = m->q_p[i]; x[NC + i] = m->xq_pi; acts[NC + i] = &m->cp_act[i]; }
        dg_fwd_entries(o.dense, qn, 2 * NC, params, x, acts, bs);
    }
    {
        CsacQminArgs& p = o.qmin;
        p = CsacQminArgs{};
        for (int i = 0; i < NC; ++i) { p.q[i] = m->cp_act[i][Lq - 1]; p.dq[i] = m->cp_dy[i][Lq - 1]; }
        p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu; p.q_min = m->pr_qmin; p.B = bs;
    }
    // dq/da: the critics' input gradients, layer by layer for all NC, the input layer without a mask, into dxa
    for (int l = Lq - 1; l >= 0; --l) {
        DenseGroupEntry e{};
        for (int i = 0; i < NC; ++i)
            e.a[i] = dg_dx_args(qn.L[l], m->q_p[i], m->cp_dy[i][l], l ? m->cp_dy[i][l - 1] : m->dxa[i], l ? m->cp_act[i][l - 1] : nullptr, bs);
        o.dense.push_back(e);
    }
    {
        CsacActorArgs& p = o.agrad;
        p = CsacActorArgs{};
        for (int i = 0; i < NC; ++i) p.dxa[i] = m->dxa[i];
        p.ldx = qn.L[0].Kp; p.NC = NC; p.O = O; p.A = A; p.B = bs; p.mlp2 = mlp2 ? 1 : 0;
        p.g_lpm = m->g_lpm; p.g_lpl = m->g_lpl; p.g_am = m->g_am; p.g_al = m->g_al; p.ent = m->ent; p.logp = m->pr_logp; p.q_min = m->pr_qmin;
        p.gout = m->p_dy[Lp - 1]; p.ldm = pn.L[Lp - 1].Np; p.gh2 = m->h2_part; p.dq_da = m->pr_dqda;
        p.scal = m->scal; p.accumulate = 0;
    }
    {   // CandleAgent::actor_step: head2 as one more segment of an Mlp3 actor
        std::vector<float*>* acts[1] = {&m->p_act}; std::vector<float*>* dys[1] = {&m->p_dy};
        const DenseReduceSeg h2seg{m->h2_part, (size_t)pad64(A), 1, (unsigned)(m->h2_off / 4), (unsigned)(pad64(A) / 4)};
        dg_step_entries(o, CS_NET_ACTOR, pn, 1, &m->pi_p, &m->pi_g, &m->pi_m, &m->pi_v, nullptr, m->x_o, acts, dys, m->pi_part, 0, m->pi_off, bs, m->pi_total,
                        cfg.critic_tau, mlp2 ? nullptr : &h2seg);
    }
    // ---- update_critic
    { const float* pp[1] = {m->pi_p}; const float* x[1] = {m->x_no}; std::vector<float*>* acts[1] = {&m->pn_act}; dg_fwd_entries(o.dense, pn, 1, pp, x, acts, bs); }
    o.sample[1] = sample(m->pn_act[Lp - 1], m->pr_next_a, m->xq_next, m->pr_nlogp, false);
    {
        const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
        for (int i = 0; i < NC; ++i) { params[i] = m->q_t[i]; x[i] = m->xq_next; acts[i] = &m->t_act[i]; }
        dg_fwd_entries(o.dense, qn, NC, params, x, acts, bs);
    }
    {
        CsacCriticArgs& p = o.closs;
        p = CsacCriticArgs{};
        for (int i = 0; i < NC; ++i) { p.q[i] = m->c_act[i][Lq - 1]; p.dq[i] = m->c_dy[i][Lq - 1]; p.qt[i] = m->t_act[i][Lq - 1]; }
        p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu;
        p.reward = r->b_reward; p.term = r->b_term; p.gamma = (float)cfg.gamma; p.ent = m->ent; p.next_logp = m->pr_nlogp; p.tgt = m->pr_tgt;
        p.loss_kind = cfg.critic_loss; p.scal = m->scal; p.accumulate = 0; p.B = bs;
    }
    {
        std::vector<float*>* acts[4]; std::vector<float*>* dys[4];
        for (int i = 0; i < NC; ++i) { acts[i] = &m->c_act[i]; dys[i] = &m->c_dy[i]; }
        dg_step_entries(o, CS_NET_CRITIC, qn, NC, m->q_p, m->q_g, m->q_m, m->q_v, m->q_t, m->xq, acts, dys, m->q_part, m->q_part_stride, m->q_off, bs, qn.total,
                        cfg.critic_tau, nullptr);
    }
}

using CandleSacActKind = CandleActKind<CandleSac>;   // group acting (candle_act_group.hpp)

// ---- what is SAC's of the group core (group_core.hpp) ----------------------------------------------------------------------------------
struct CandleSacGroupKind : DenseRound<2, CS_K_DW, CS_K_REDUCE_ADAM> {
    using Member = CandleSac; using Shape = CsShape; using Launch = CsLaunch; using Step = CsacStep; using MemberArgs = CsacMemberArgs; using PlanMember = CsMember;
    using Act = CandleSacActKind;
    static constexpr const char *KIND = "candle_sac", *A = "a candle SAC", *NAME = "SAC (candle)", *CAP_MSG = "cap_per_member must hold the three keys of a SAC record";
    static constexpr int MAX_LAUNCHES = CS_MAX_LAUNCHES, K_GATHER = CS_K_GATHER, FORM = BDR_GROUP_FORM_CANDLE_SAC_LAYERS, MIN_CAP = CandleSac::N_RECORD;
    static CsMember describe(const CandleSac* m) { return CsMember{csac_shape(m), 1, m->cfg.n_updates_per_opt, m->device, m->prof ? 1 : 0, m->grad_comm ? 1 : 0, m}; }
    static int refusal(const CsMember* m, unsigned n, const char** why, int* kernel) { return cs_group_refusal(m, n, why, kernel); }
    static const char* kernel_name(int k) { return cs_kernel_name(k); }
    static int round_plan(const CsShape& s, unsigned P, CsLaunch* out) { return cs_round_plan(s, P, out); }
    static int launch_count(const CsShape& s) { return cs_launch_count(s.critic.n_layers, s.actor.n_layers); }
    // CandleAgent::opt / CandleSac::update on the host, in their order: the mode now, the draws of a (sample_elem), the entropy
    // coefficient's step (Auto only), the actor's step, the draws of next_a, the critics' step, n_opts, last_B
    static CsacStep fill_step(CandleSac* m, int bs, const GatherArgs& plan)
    {
        CsacStep st{};
        st.word_pos = plan.word_pos; st.size = plan.size;
        st.train = m->train ? 1 : 0;
        if (st.train)
            for (int d = 0; d < 2; ++d) { st.counter[d] = m->noise_counter; m->noise_counter += (uint64_t)bs * m->A; }
        if (m->cfg.ent_coef_mode == BDR_ENT_COEF_AUTO) {
            m->step_al += 1;
            st.adam[CS_ADAM_ALPHA] = adam_scalars_for(true, m->cfg.ent_coef_lr, 0.9, 0.999, 1e-8, 0.01, m->step_al);   // candle-nn ParamsAdamW::default()
        }
        m->step_pi += 1;
        st.adam[CS_NET_ACTOR] = DenseAgent::opt_scalars(m->cfg.opt_actor, m->cfg.lr_actor, m->step_pi);
        m->step_q += 1;
        st.adam[CS_NET_CRITIC] = DenseAgent::opt_scalars(m->cfg.opt_critic, m->cfg.lr_critic, m->step_q);
        m->n_opts += 1;
        m->last_B = bs;
        return st;
    }
    static void member_static(CandleSac* m, int bs, const bdr_replay* r, const GatherArgs& plan, CsacMemberArgs& o) { csac_member_static(m, bs, r, plan, o); }

    static constexpr DgReduceEntry<CsacStep> RA[] = {k_csac_reduce_adam_group<CS_NET_ACTOR>, k_csac_reduce_adam_group<CS_NET_CRITIC>};
    StagedArray<CsacPackArgs> pack; StagedArray<CsacAlphaArgs> alpha; StagedArray<CsacQminArgs> qmin; StagedArray<CsacActorArgs> agrad;   // [P]
    StagedArray<CsacCriticArgs> closs;                                                                                                    // [P]
    StagedArray<CsacSampleArgs> sample;                                                                                                   // [2][P]: a, next_a
    hipError_t allocate(const CsShape& s, size_t P)
    {
        return allocate_round(cs_dense_launches(s.critic.n_layers, s.actor.n_layers), P, pack, [&] {
            const hipError_t e = staged_resize(P, alpha, qmin, agrad, closs);
            return e == hipSuccess ? sample.resize(2 * P) : e;
        });
    }
    // member p's arguments into the staging arrays
    void stage(size_t p, size_t P, const CsacMemberArgs& o)
    {
        stage_dense(p, P, o);
        pack[p] = o.pack; alpha[p] = o.alpha; qmin[p] = o.qmin; agrad[p] = o.agrad; closs[p] = o.closs;
        for (int d = 0; d < 2; ++d) sample[(size_t)d * P + p] = o.sample[d];
    }
    hipError_t upload() { return staged_upload(gather, pack, dense, sample, alpha, qmin, agrad, closs, dw, ra); }
    int32_t launch(const GroupCore<CandleSacGroupKind>& g, size_t P, const CsacStep* steps_dev, unsigned seq_no) const { return dg_round_launch(g, P, steps_dev, seq_no, *this); }
    // SAC's own launches of a round
    int32_t launch_own(const CsLaunch& l, int n, size_t P, dim3 grid, dim3 block, const BDR_CONST_AS CsacStep* st, hipStream_t stream) const
    {
        switch (l.kernel) {
        case CS_K_PACK: hipLaunchKernelGGL(k_csac_pack_group, grid, block, 0, stream, (const BDR_CONST_AS CsacPackArgs*)pack.d.get()); break;
        case CS_K_SAMPLE_LOGP:
            BDR_REQUIRE(l.layer == 0 || l.layer == 1, "SAC group round: launch %d of the plan names no draw", n);
            hipLaunchKernelGGL(k_csac_sample_logp_group, grid, block, 0, stream, (const BDR_CONST_AS CsacSampleArgs*)(sample.d.get() + (size_t)l.layer * P), st, l.layer);
            break;
        case CS_K_ALPHA: hipLaunchKernelGGL(k_csac_alpha_group, grid, block, 0, stream, (const BDR_CONST_AS CsacAlphaArgs*)alpha.d.get(), st); break;
        case CS_K_QMIN: hipLaunchKernelGGL(k_csac_qmin_group, grid, block, 0, stream, (const BDR_CONST_AS CsacQminArgs*)qmin.d.get()); break;
        case CS_K_ACTOR_GRAD: hipLaunchKernelGGL(k_csac_actor_grad_group, grid, block, 0, stream, (const BDR_CONST_AS CsacActorArgs*)agrad.d.get()); break;
        case CS_K_CRITIC_LOSS: hipLaunchKernelGGL(k_csac_critic_loss_group, grid, block, 0, stream, (const BDR_CONST_AS CsacCriticArgs*)closs.d.get()); break;
        default: return fail(BDR_ERR_INVALID, "SAC group round: launch %d of the plan names no kernel", n);
        }
        return BDR_OK;
    }
};

}  // namespace

struct bdr_candle_sac_group : GroupCore<CandleSacGroupKind> {};

namespace bdr {
int candle_sac_group_act_dim(const void* group, uint32_t member) { return group_act_dim<bdr_candle_sac_group>(group, member); }   // (trainer.hip)
int candle_sac_group_obs_dim(const void* group, uint32_t member) { return group_obs_dim<bdr_candle_sac_group>(group, member); }   // (trainer.hip)
}  // namespace bdr

extern "C" {

int32_t bdr_candle_sac_group_create(bdr_agent* const* agents, uint32_t n, bdr_candle_sac_group** out) { return group_create(agents, n, out); }
int32_t bdr_candle_sac_group_destroy(bdr_candle_sac_group* g) { return group_destroy(g); }
int32_t bdr_candle_sac_group_size(const bdr_candle_sac_group* g, uint32_t* n) { return group_size(g, n); }
int32_t bdr_candle_sac_group_member(const bdr_candle_sac_group* g, uint32_t i, bdr_agent** out) { return group_member(g, i, out); }
int32_t bdr_candle_sac_group_info(const bdr_candle_sac_group* g, bdr_group_info* out) { return group_info(g, out); }
int32_t bdr_candle_sac_group_opt(bdr_candle_sac_group* g, bdr_replay* const* buffers) { return group_opt(g, buffers); }
int32_t bdr_candle_sac_group_opt_with_scalars(bdr_candle_sac_group* g, bdr_replay* const* buffers, float* out, int32_t cap_per_member, int32_t* n_out)
{
    return group_opt_with_scalars(g, buffers, out, cap_per_member, n_out);
}
int32_t bdr_candle_sac_group_sample(bdr_candle_sac_group* g, const bdr_obs_norm* const* norms, uint64_t n, const void* const* rows, const int32_t* dtypes,
                                    float* const* act_out)
{
    return group_sample(g, norms, n, rows, dtypes, act_out);
}
int32_t bdr_candle_sac_group_sample_members(bdr_candle_sac_group* g, const uint32_t* members, uint32_t n_sel, const bdr_obs_norm* const* norms, uint64_t n,
                                            const void* const* rows, const int32_t* dtypes, float* const* act_out)
{
    return group_sample_members(g, members, n_sel, norms, n, rows, dtypes, act_out);
}
int32_t bdr_candle_sac_group_sync(bdr_candle_sac_group* g) { return group_sync(g); }
int32_t bdr_candle_sac_group_copy_members(bdr_candle_sac_group* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags)
{
    return group_copy_members(g, src, dst, n, flags);
}
int32_t bdr_candle_sac_group_push(bdr_candle_sac_group* g, bdr_replay* const* buffers, uint64_t n, const void* const* obs, const void* const* next_obs, const int32_t* obs_dtypes,
        const float* const* act, const float* const* reward, const int8_t* const* is_terminated, const int8_t* const* is_truncated)
{
    return group_push(g, buffers, n, obs, next_obs, obs_dtypes, act, reward, is_terminated, is_truncated);
}
int32_t bdr_candle_sac_group_push_max_rows(bdr_candle_sac_group* g, bdr_replay* const* buffers, const int32_t* obs_dtypes, uint64_t* n_max)
{
    return group_push_max_rows(g, buffers, obs_dtypes, n_max);
}

}  // extern "C"
