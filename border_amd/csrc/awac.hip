// AWAC agent on MI355X: Awac::opt_ (border-candle-agent/src/awac/base.rs:170-215) with update_actor (:127-168) and then
// update_critic (:66-125) on the same batch; critics = MultiCritic of Mlp on cat(obs, act) (util/critic.rs), actor = GaussianActor
// (util/actor.rs) over Mlp3 (mlp/mlp3.rs).  No value network.
// Dense layers run on the FP32-MFMA kernels of dense.hpp (unchanged); Policy::sample is candle_actor.hpp's k_candle_sample, written
// straight into the action columns of a critic input.  AWAC's own math is the three kernels below:
//   k_awac_pack          the batch rows -> the actor and critic inputs
//   k_awac_actor_loss    min over the ONLINE critics on (obs, act) and (obs, act_), adv, w, logp, dL/dmean and dL/dhead2; one
//                        workgroup per action dimension forms that dimension's head2 sum, all of them concurrently, and one more
//                        workgroup the per-row outputs, the loss and the record sums
//   k_awac_critic_loss   TD target from the target critics on (next_obs, next_act), the SUM over critics of the per-critic losses
// Every batch-wide sum is formed in one fixed order (candle_actor.hpp), so an update gives the same bits run to run.
// Noise order: in train mode each update takes B*A draws of the agent's counter stream for act_ (row-major [B][A]), then B*A for
// next_act - the stream bdr_agent_draw_noise reads.  Host-given draws (bdr_awac_update_on_batch's z_pi / z_next) take none.  Eval
// mode uses the means and no draws.
// Reference quirks kept on purpose: gamma_not_done counts is_truncated (util.rs:235-255); the Tanh limit's log-Jacobian uses the
// action itself (util/actor.rs:210-218); only the first five record values are averaged over n_updates_per_opt (awac/base.rs:190-196);
// MultiCritic::save writes the ONLINE critics into critic.tgt.pt and load reads both files into the online critics (util/critic.rs:272-298).
#include <algorithm>
#include <cstdlib>

#include "candle_actor.hpp"

using namespace bdr;

namespace {

// obs / next_obs / act rows -> the zero-padded actor inputs ([B][Kp]: obs, next_obs) and the three critic inputs ([B][Kq]): (obs | act),
// and the observation columns of (obs | act_) and (next_obs | next_act), whose action columns k_candle_sample fills
struct AwacPackArgs { const float* obs; const float* next; const float* act; int O, A, B; float* x_o; float* x_no; int ldp; float* xq; float* xq_pi; float* xq_next; int ldq; };
// (the bodies of the three kernels below are functions over their argument struct: the kernel argument, or a member's entry of a device
// array read in place - awac_group.hpp, where blockIdx.y is the member; `red` is the kernel's own 32 floats of LDS)
template <class Args>
__device__ __forceinline__ void awac_pack_body(const Args& p)
{
    const int W = p.O + p.A;
    const size_t n = (size_t)p.B * W;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) {
        const int b = (int)(t / W), c = (int)(t % W);
        const size_t q = (size_t)b * p.ldq + c;
        if (c < p.O) {
            const float o = p.obs[(size_t)b * p.O + c];
            const float nx = p.next[(size_t)b * p.O + c];
            p.x_o[(size_t)b * p.ldp + c] = o;
            p.x_no[(size_t)b * p.ldp + c] = nx;
            p.xq[q] = o; p.xq_pi[q] = o; p.xq_next[q] = nx;
        } else {
            p.xq[q] = p.act[(size_t)b * p.A + (c - p.O)];
        }
    }
}
__global__ __launch_bounds__(256) void k_awac_pack(AwacPackArgs p) { awac_pack_body(p); }

// update_actor (awac/base.rs:127-168): q = min_i Q_i(obs, act), v = min_i Q_i(obs, act_) (online critics, util/critic.rs:197-202),
// adv = q - v; w = clamp(exp(inv_lambda adv), 0, exp_adv_max) or softmax(inv_lambda adv) over the batch; logp of the batch actions
// under N(mean, std^2), std = exp(clamp(head2, min, max)) (util/actor.rs:196-223; Tanh limit: x = atanh(clamp(a / scale)) plus the
// log-Jacobian of `a`); loss = mean(-logp w).  Gradients: dL/dmean = -(w/B) (x - mean) / var and
// dL/dhead2_j = sum_b -(w_b/B)(-1 + (x - mean)^2 / var) where min <= head2_j <= max (0 outside: the clamp).
// Grid: A + 1 workgroups.  Workgroup j < A: column j of dL/dmean and the head2_j sum.  Workgroup A: the per-row probes, the loss and
// the record sums.  Each workgroup forms w the same way from the same inputs (the softmax's max and sum included), so they agree bit
// for bit.
struct AwacActorArgs {
    const float* qd[4]; const float* qp[4]; int ldq; int NC;   // Q_i(obs, act), Q_i(obs, act_): column 0 of [B][ldq]
    const float* mean; int ldm; const float* head2; const float* act; int A;
    float lo, hi; int tanh_limit; float scale;
    float inv_lambda, exp_adv_max; int softmax;
    float* q_data; float* q_pi; float* adv; float* w; float* logp;   // probes [B]
    float* gmean; float* gh2;                                        // [B][ldm], [A]
    float* scal; int accumulate; int B;                              // scal[1] loss_actor, [3] adv_mean, [4] adv_abs_mean, [5] logp_mean
};
template <class Args>
__device__ __forceinline__ float awac_x(const Args& p, float a)
{
#pragma clang fp contract(off)
    if (!p.tanh_limit) return a;
    const float t = fminf(fmaxf(a / p.scale, -0.999999f), 0.999999f);   // util.rs:268-271 atanh
    const float r = (1.0f + t) / (1.0f - t);
    return 0.5f * logf(r);
}
struct AwacAdv { float q, v, adv, z; };
template <class Args>
__device__ __forceinline__ AwacAdv awac_adv(const Args& p, int b)
{
#pragma clang fp contract(off)
    AwacAdv r;
    r.q = p.qd[0][(size_t)b * p.ldq];
    r.v = p.qp[0][(size_t)b * p.ldq];
    for (int i = 1; i < p.NC; ++i) { r.q = fminf(r.q, p.qd[i][(size_t)b * p.ldq]); r.v = fminf(r.v, p.qp[i][(size_t)b * p.ldq]); }
    r.adv = r.q - r.v;
    r.z = r.adv * p.inv_lambda;
    return r;
}
template <class Args>
__device__ __forceinline__ void awac_actor_loss_body(const Args& p, float* red)
{
    const float invB = 1.0f / (float)p.B;
    // softmax(z, 0) = exp(z - max) / sum(exp(z - max)): one batch-wide max and sum per workgroup
    float mx = 0.f, se = 1.f;
    if (p.softmax) {
        mx = candle::row_max(p.B, [&](int b) { return awac_adv(p, b).z; }, red);
        se = candle::row_sum(p.B, [&](int b) { return expf(awac_adv(p, b).z - mx); }, red);
    }
    auto weight = [&](float z) { return p.softmax ? expf(z - mx) / se : fminf(fmaxf(expf(z), 0.0f), p.exp_adv_max); };
    const int j = blockIdx.x;
    if (j < p.A) {
        const float h = p.head2[j];
        const float sd = expf(fminf(fmaxf(h, p.lo), p.hi));
        const float var = sd * sd;
        const float s = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
            const float wb = weight(awac_adv(p, b).z);
            const float gl = -wb * invB;   // dL/dlogp_b
            const float d = awac_x(p, p.act[(size_t)b * p.A + j]) - p.mean[(size_t)b * p.ldm + j];
            p.gmean[(size_t)b * p.ldm + j] = gl * (d / var);
            const float r = (d * d) / var - 1.0f;
            return -(wb * invB) * r;
        }, red);
        if (threadIdx.x == 0) p.gh2[j] = (h >= p.lo && h <= p.hi) ? s : 0.f;
        return;
    }
    // per row: q, v, adv, w, logp; the loss and the record sums
    const float s_wl = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
        const AwacAdv r = awac_adv(p, b);
        const float wb = weight(r.z);
        float lp = 0.f, lj = 0.f;
        for (int k = 0; k < p.A; ++k) {
            const float ls = fminf(fmaxf(p.head2[k], p.lo), p.hi);
            const float sd = expf(ls);
            const float var = sd * sd;
            const float a = p.act[(size_t)b * p.A + k];
            const float x = awac_x(p, a);
            const float d = x - p.mean[(size_t)b * p.ldm + k];
            const float hl = 0.5f * logf(var);
            const float q = (0.5f / var) * (d * d);
            const float t0 = -0.91893853320467274178f - hl;
            lp += t0 - q;
            if (p.tanh_limit) { const float ac = fminf(fmaxf(a, -0.999999f), 0.999999f); lj += logf(1.0f - ac * ac); }
        }
        const float l = p.tanh_limit ? lp - lj : lp;
        p.q_data[b] = r.q; p.q_pi[b] = r.v; p.adv[b] = r.adv; p.w[b] = wb; p.logp[b] = l;
        return wb * l;
    }, red);
    // a thread reads back only the rows it wrote itself
    const float s_adv = candle::row_sum(p.B, [&](int b) { return p.adv[b]; }, red);
    const float s_abs = candle::row_sum(p.B, [&](int b) { return fabsf(p.adv[b]); }, red);
    const float s_lp = candle::row_sum(p.B, [&](int b) { return p.logp[b]; }, red);
    if (threadIdx.x == 0) {
        const int acc = p.accumulate;
        p.scal[1] = candle::acc(acc ? p.scal[1] : 0.f, -s_wl, invB);
        p.scal[3] = candle::acc(acc ? p.scal[3] : 0.f, s_adv, invB);
        p.scal[4] = candle::acc(acc ? p.scal[4] : 0.f, s_abs, invB);
        p.scal[5] = candle::acc(acc ? p.scal[5] : 0.f, s_lp, invB);
    }
}
__global__ __launch_bounds__(1024) void k_awac_actor_loss(AwacActorArgs p)
{
    __shared__ float red[32];
    awac_actor_loss_body(p, red);
}

// update_critic (awac/base.rs:66-125): next_q = min_i Qtgt_i(next_obs, next_act), tgt = r + gamma_not_done * next_q with
// gamma_not_done = (1 - (term | trunc)) * gamma in f32 (util.rs:235-255); loss = sum_i mean_b loss(Q_i - tgt), MSE or smooth L1
// (util.rs:144-152); dL/dQ_i = loss'(Q_i - tgt) / B (masked by the output ReLU when the critic Mlp has one).  Record sums:
// scal[0] loss_critic, [2] mean |tgt|, [6] mean r, [7] mean next_q.
struct AwacCriticArgs {
    const float* q[4]; float* dq[4]; const float* qt[4]; int ldq; int NC; int relu_out;
    const float* reward; const int8_t* term; const int8_t* trunc; float gamma;
    float* tgt; float* next_q;   // [B]
    int loss_kind; float* scal; int accumulate; int B;
};
template <class Args>
__device__ __forceinline__ void awac_critic_loss_body(const Args& p, float* red)
{
    const float invB = 1.0f / (float)p.B;
    const float s_abs = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
        float nq = p.qt[0][(size_t)b * p.ldq];
        for (int i = 1; i < p.NC; ++i) nq = fminf(nq, p.qt[i][(size_t)b * p.ldq]);
        const float done = (float)(p.term[b] | p.trunc[b]);
        const float gnd = (1.0f - done) * p.gamma;
        const float c = gnd * nq;
        const float t = p.reward[b] + c;
        p.tgt[b] = t; p.next_q[b] = nq;
        return fabsf(t);
    }, red);
    // a thread reads back only the targets it wrote itself
    const float s_r = candle::row_sum(p.B, [&](int b) { return p.reward[b]; }, red);
    const float s_nq = candle::row_sum(p.B, [&](int b) { return p.next_q[b]; }, red);
    float total = 0.f;
    for (int i = 0; i < p.NC; ++i) {   // critic by critic, summed in critic order (Tensor::stack(..).sum_all())
        const float si = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
            const float q = p.q[i][(size_t)b * p.ldq];
            const float d = q - p.tgt[b];
            float l, g;
            candle::critic_loss_elem(p.loss_kind, d, l, g);
            float gq = g * invB;
            if (p.relu_out && !(q > 0.f)) gq = 0.f;
            p.dq[i][(size_t)b * p.ldq] = gq;
            return l;
        }, red);
        total = candle::acc(total, si, invB);
    }
    if (threadIdx.x == 0) {
        const int acc = p.accumulate;
        p.scal[0] = (acc ? p.scal[0] : 0.f) + total;
        p.scal[2] = candle::acc(acc ? p.scal[2] : 0.f, s_abs, invB);
        p.scal[6] = candle::acc(acc ? p.scal[6] : 0.f, s_r, invB);
        p.scal[7] = candle::acc(acc ? p.scal[7] : 0.f, s_nq, invB);
    }
}
__global__ __launch_bounds__(1024) void k_awac_critic_loss(AwacCriticArgs p)
{
    __shared__ float red[32];
    awac_critic_loss_body(p, red);
}

}  // namespace


// ================================================================================================
// The actor, the critics and their steps, Policy::sample, the parameter views and the checkpoints are CandleAgent's
// (candle_actor.hpp); AWAC adds its update schedule, the sampled actions' critic inputs and the host noise rows of update_on_batch.
struct Awac : CandleAgent<Awac, bdr_awac_config> {
    static constexpr const char* NAME = "AWAC";
    static constexpr int N_RECORD = 8;   // scal: the 8 record values, summed over the updates of one opt (see record())
    // batch buffers
    float *xq_pi = nullptr, *xq_next = nullptr;               // critic inputs (obs | act_), (next_obs | next_act)
    std::vector<float*> pn_act;                               // the updated actor on next_obs
    std::vector<float*> cp_act[4];                            // critics on (obs, act_); the targets on (next_obs, next_act) are t_act
    float *pr_qd = nullptr, *pr_qp = nullptr, *pr_adv = nullptr, *pr_nq = nullptr;
    float *pr_act = nullptr, *pr_next_act = nullptr;          // [B][A]
    float* u_z = nullptr;                                     // host noise rows of update_on_batch: z_pi | z_next

    int32_t alloc_batch(int Bn)
    {
        for (auto p : {&xq_pi, &xq_next}) BDR_TRY(alloc(p, (size_t)Bn * qn.L[0].Kp, BATCH));
        BDR_TRY(layer_bufs(pn, Bn, pn_act));
        for (int i = 0; i < NC; ++i) BDR_TRY(layer_bufs(qn, Bn, cp_act[i]));
        for (auto p : {&pr_qd, &pr_qp, &pr_adv, &pr_nq}) BDR_TRY(alloc(p, Bn, BATCH));
        for (auto p : {&pr_act, &pr_next_act}) BDR_TRY(alloc(p, (size_t)Bn * A, BATCH));
        return BDR_OK;
    }
    int32_t alloc_staging(uint64_t n) { return alloc(&u_z, 2 * n * A, STAGING, false); }
    double* own_hyper(int32_t id) { return id == BDR_HYPER_INV_LAMBDA ? &cfg.inv_lambda : id == BDR_HYPER_EXP_ADV_MAX ? &cfg.exp_adv_max : nullptr; }

    // One iteration of the Awac::opt_ loop on device-resident rows (f32 obs / next_obs / act).  z_pi / z_next: device N(0,1) rows or null.
    int32_t update(int Bn, const float* obs, const float* act, const float* next_obs, const float* reward, const int8_t* term,
                   const int8_t* trunc, bool first, const float* z_pi = nullptr, const float* z_next = nullptr)
    {
        BDR_TRY(ensure_batch(Bn));
        const int Lq = (int)qn.L.size(), Lp = (int)pn.L.size();
        const int ldq = qn.L[Lq - 1].Np;
        {
            AwacPackArgs p{obs, next_obs, act, O, A, Bn, x_o, x_no, pn.L[0].Kp, xq, xq_pi, xq_next, qn.L[0].Kp};
            const size_t n = (size_t)Bn * (O + A);
            Bracket br(this, "pack");
            BDR_HIP(step_launch(stream, true, k_awac_pack, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), p));
        }
        // ---------------- update_actor (:127-168) ----------------
        BDR_TRY(actor_forward(x_o, p_act, Bn));
        BDR_TRY(sample_pack(p_act[Lp - 1], Bn, z_pi, pr_act, xq_pi, "awac_sample_pack"));   // act_ = actor.sample(obs) (:133)
        // the online critics on (obs, act) and (obs, act_): 2 NC pairs.  No critic parameter changes before update_critic, so the
        // (obs, act) activations are also that step's predictions and activations.
        {
            const float* params[8]; const float* x[8]; std::vector<float*>* acts[8];
            for (int i = 0; i < NC; ++i) { params[i] = q_p[i]; x[i] = xq; acts[i] = &c_act[i]; params[NC + i] = q_p[i]; x[NC + i] = xq_pi; acts[NC + i] = &cp_act[i]; }
            BDR_TRY(mlp_forward(qn, 2 * NC, params, x, acts, Bn, "q_fwd"));
        }
        {
            AwacActorArgs p{};
            for (int i = 0; i < NC; ++i) { p.qd[i] = c_act[i][Lq - 1]; p.qp[i] = cp_act[i][Lq - 1]; }
            p.ldq = ldq; p.NC = NC;
            p.mean = p_act[Lp - 1]; p.ldm = pn.L[Lp - 1].Np; p.head2 = pi_p + h2_off; p.act = act; p.A = A;
            p.lo = (float)cfg.min_log_std; p.hi = (float)cfg.max_log_std; p.tanh_limit = cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
            p.scale = (float)cfg.action_scale; p.inv_lambda = (float)cfg.inv_lambda; p.exp_adv_max = (float)cfg.exp_adv_max; p.softmax = cfg.adv_softmax ? 1 : 0;
            p.q_data = pr_qd; p.q_pi = pr_qp; p.adv = pr_adv; p.w = pr_w; p.logp = pr_logp; p.gmean = p_dy[Lp - 1]; p.gh2 = h2_part;
            p.scal = scal; p.accumulate = first ? 0 : 1; p.B = Bn;
            Bracket br(this, "awac_actor_loss");
            BDR_HIP(step_launch(stream, false, k_awac_actor_loss, dim3(A + 1), dim3(1024), p));
        }
        BDR_TRY(actor_step(Bn));
        // ---------------- update_critic (:66-125) ----------------
        // next_act = actor.sample(next_obs) from the UPDATED actor (:85)
        BDR_TRY(actor_forward(x_no, pn_act, Bn));
        BDR_TRY(sample_pack(pn_act[Lp - 1], Bn, z_next, pr_next_act, xq_next, "awac_sample_pack"));
        {
            const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
            for (int i = 0; i < NC; ++i) { params[i] = q_t[i]; x[i] = xq_next; acts[i] = &t_act[i]; }
            BDR_TRY(mlp_forward(qn, NC, params, x, acts, Bn, "q_tgt_fwd"));
        }
        {
            AwacCriticArgs p{};
            for (int i = 0; i < NC; ++i) { p.q[i] = c_act[i][Lq - 1]; p.dq[i] = c_dy[i][Lq - 1]; p.qt[i] = t_act[i][Lq - 1]; }
            p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu;
            p.reward = reward; p.term = term; p.trunc = trunc; p.gamma = (float)cfg.gamma; p.tgt = pr_tgt; p.next_q = pr_nq;
            p.loss_kind = cfg.critic_loss; p.scal = scal; p.accumulate = first ? 0 : 1; p.B = Bn;
            Bracket br(this, "awac_critic_loss");
            BDR_HIP(step_launch(stream, false, k_awac_critic_loss, dim3(1), dim3(1024), p));
        }
        BDR_TRY(critic_step(Bn));
        n_opts += 1;
        last_B = Bn;
        return BDR_OK;
    }

    const char* kind() const override { return "awac"; }
    void record_keys(std::vector<std::string>& keys) override
    {
        keys = {"loss_critic", "loss_actor", "q_tgt_abs_mean", "adv_mean", "adv_abs_mean", "logp_mean", "reward_mean", "next_q_mean"};
    }
    int32_t record(float* out, int cap, int* n) override
    {
        float h[8];
        BDR_HIP(hipMemcpyAsync(h, scal, 32, hipMemcpyDeviceToHost, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        if (cap < 8) return fail(BDR_ERR_INVALID, "AWAC record needs 8 slots");
        // awac/base.rs:190-196: the first five are divided by n_updates_per_opt; logp_mean, reward_mean, next_q_mean stay sums
        const float nu = (float)cfg.n_updates_per_opt;
        for (int k = 0; k < 8; ++k) out[k] = k < 5 ? h[k] / nu : h[k];
        *n = 8;
        return BDR_OK;
    }
};

namespace {
constexpr const char* kOneRow =
    "AWAC needs at least 2 rows per batch: at one row the reference squeezes the critic minima and the TD target to scalars while each "
    "prediction keeps shape [1], and candle's same-shape tensor ops reject that pair (awac/base.rs:88, util/critic.rs:197-218)";
}  // namespace

extern "C" {

void bdr_awac_config_default(bdr_awac_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    // awac/config.rs:120-141
    c->gamma = 0.99; c->inv_lambda = 10.0; c->exp_adv_max = 100.0; c->n_updates_per_opt = 1; c->batch_size = 1; c->adv_softmax = 0;
    c->critic_loss = BDR_LOSS_MSE; c->device = -1; c->train = 0;
    // MultiCriticConfig (util/critic.rs:35-43), GaussianActorConfig (util/actor.rs:44-55)
    c->n_critics = 2; c->critic_tau = 0.005;
    c->lr_actor = c->lr_critic = 3e-4;
    c->min_log_std = -20.0; c->max_log_std = 2.0;
    c->action_limit = BDR_ACTION_LIMIT_CLAMP; c->action_min = -1.0; c->action_max = 1.0; c->action_scale = 1.0;
    for (bdr_adamw_config* o : {&c->opt_actor, &c->opt_critic}) { o->opt_kind = BDR_OPT_ADAM; o->beta1 = 0.9; o->beta2 = 0.999; o->weight_decay = 0.01; o->eps = 1e-8; }
    for (bdr_mlp_config* m : {&c->actor, &c->critic}) m->activation_out = BDR_ACTIVATION_NONE;
}

int32_t bdr_awac_create(const bdr_awac_config* cfg, bdr_agent** out)
{
    BDR_REQUIRE(cfg && out, "null argument");
    return Awac::create(*cfg, out, nullptr, nullptr, kOneRow);
}

int32_t bdr_awac_update_on_batch(bdr_agent* base, uint64_t n, const float* obs, const float* act, const float* next_obs,
                                 const float* reward, const int8_t* term, const int8_t* trunc, const float* z_pi, const float* z_next, float* rec8)
{
    BDR_REQUIRE(base && obs && act && next_obs && reward && term && trunc, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "awac"), "not an AWAC agent");
    BDR_REQUIRE(n != 1, "%s", kOneRow);
    BDR_REQUIRE(n >= 2 && n <= 65536, "batch size out of range");
    Awac* a = static_cast<Awac*>(base);
    BDR_TRY(a->stage_batch(n, obs, act, next_obs, reward, term, trunc));
    float* dz_pi = nullptr; float* dz_next = nullptr;
    if (z_pi) { dz_pi = a->u_z; BDR_HIP(hipMemcpyAsync(dz_pi, z_pi, n * a->A * 4, hipMemcpyHostToDevice, a->stream)); }
    if (z_next) { dz_next = a->u_z + n * a->A; BDR_HIP(hipMemcpyAsync(dz_next, z_next, n * a->A * 4, hipMemcpyHostToDevice, a->stream)); }
    BDR_TRY(a->update((int)n, a->u_obs, a->u_act, a->u_next, a->u_rew, a->u_term, a->u_trunc, true, dz_pi, dz_next));
    return a->batch_done(rec8);
}

// Parity probes of the LAST update (see include/border_amd.h)
int32_t bdr_awac_probe(bdr_agent* base, int32_t what, float* out, uint64_t n)
{
    BDR_REQUIRE(base && out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "awac"), "not an AWAC agent");
    Awac* a = static_cast<Awac*>(base);
    BDR_HIP(hipSetDevice(a->device));
    const int Bn = a->last_B, NC = a->NC;
    BDR_REQUIRE(Bn > 0, "no update has run yet");
    BDR_HIP(hipStreamSynchronize(a->stream));
    if (what < 0 || what > 9) return fail(BDR_ERR_INVALID, "unknown AWAC probe %d", what);
    if (what == 9) {   // Q_i(obs, act): column 0 of the critics' last layer
        BDR_REQUIRE(n == (uint64_t)NC * Bn, "q_pred holds n_critics x batch values");
        const int Lq = (int)a->qn.L.size(), ld = a->qn.L[Lq - 1].Np;
        std::vector<float> h((size_t)Bn * ld);
        for (int i = 0; i < NC; ++i) {
            BDR_HIP(hipMemcpy(h.data(), a->c_act[i][Lq - 1], h.size() * 4, hipMemcpyDeviceToHost));
            for (int b = 0; b < Bn; ++b) out[(size_t)i * Bn + b] = h[(size_t)b * ld];
        }
        return BDR_OK;
    }
    if (what == 5 || what == 6) {
        BDR_REQUIRE(n == (uint64_t)Bn * a->A, "this probe holds batch x act_dim values");
        BDR_HIP(hipMemcpy(out, what == 5 ? a->pr_act : a->pr_next_act, n * 4, hipMemcpyDeviceToHost));
        return BDR_OK;
    }
    const float* rows[10] = {a->pr_qd, a->pr_qp, a->pr_adv, a->pr_w, a->pr_logp, nullptr, nullptr, a->pr_nq, a->pr_tgt, nullptr};
    BDR_REQUIRE(n == (uint64_t)Bn, "this probe holds batch values");
    BDR_HIP(hipMemcpy(out, rows[what], (size_t)Bn * 4, hipMemcpyDeviceToHost));
    return BDR_OK;
}

// Policy::sample (util/actor.rs:226-241); out: [n][act_dim]
int32_t bdr_awac_sample(bdr_agent* base, uint64_t n, const float* obs, float* act_out)
{
    BDR_REQUIRE(base && obs && act_out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "awac"), "not an AWAC agent");
    return static_cast<Awac*>(base)->sample(n, obs, act_out);
}

int32_t bdr_awac_sample_device(bdr_agent* base, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out)
{
    BDR_REQUIRE(base && obs_dev && act_out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "awac"), "not an AWAC agent");
    return static_cast<Awac*>(base)->sample_device(n, obs_dev, row_stride, act_out);
}

}  // extern "C"

// the launch grouping of AWAC agents (bdr_awac_group_*): it needs Awac and the kernel bodies above
#include "awac_group.hpp"
