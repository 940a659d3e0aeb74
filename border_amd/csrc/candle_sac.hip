// SAC agent of border-candle-agent on MI355X: Sac::opt_ (border-candle-agent/src/sac/base.rs:124-134) with update_actor (:104-122)
// and then update_critic (:63-102) on the same batch, the already updated actor and alpha; critics = MultiCritic of Mlp on
// cat(obs, act) (util/critic.rs), actor = GaussianActor (util/actor.rs) over Mlp3 (mlp/mlp3.rs) or Mlp2 (mlp/mlp2.rs), the
// entropy coefficient EntCoef (sac/ent_coef.rs).  Not sac.hip, which restates border-tch-agent's SAC.
// Dense layers run on the FP32-MFMA kernels of dense.hpp (unchanged).  SAC's own math is the kernels below:
//   k_csac_pack          the batch rows -> the actor and critic inputs
//   k_csac_sample_logp   a = Policy::sample from the actor's last layer, logp of that same a, and (gradient form) the per-element
//                        total derivatives of logp and of a with respect to the mean and to the second output; a group of lanes per row
//   k_csac_alpha         the fixed-order mean of logp, the AdamW step of log_alpha, the new alpha
//   k_csac_qmin          q = min_i Q_i(obs, a) and dQ_i = -[Q_i == q] / B, the output gradient of the critics' input-gradient chain
//   k_csac_actor_grad    dL/dmean, dL/d(second output) and loss_actor from the partials and dq/da
//   k_csac_critic_loss   the TD target, the MEAN over critics of the per-critic losses, dQ_i
// Every batch-wide sum is formed in one fixed order (candle_actor.hpp), so an update gives the same bits run to run.
// Noise order: in train mode each update takes B*A draws of the agent's counter stream for a (row-major [B][A]), then B*A for
// next_a - the stream bdr_agent_draw_noise reads.  Host-given draws (z_pi / z_next) take none.  Eval mode uses the means, no draws.
// Reference quirks kept on purpose: Mlp2's double exponential (std = exp(clamp(exp(s)))); the Tanh limit's log-Jacobian uses the
// action itself, not a / scale (util.rs:274-279); is_truncated is ignored (gamma_not_done(.., None, ..), sac/base.rs:75-76);
// MultiCritic::save writes the ONLINE critics into critic.tgt.pt and load reads both files into the online critics.
// Clamp gradients: closed ranges with gradient 1 on the bounds (tests/edge_inputs.py), for the log-std clamp, the Clamp limit,
// atanh's clamp and the Jacobian's clamp.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "candle_actor.hpp"

using namespace bdr;

namespace {

// obs / next_obs / act rows -> the zero-padded actor inputs ([B][Kp]: obs, next_obs) and the critic inputs ([B][Kq]): (obs | act), and
// the observation columns of (obs | a) and (next_obs | next_a), whose action columns k_csac_sample_logp fills.
// Bounds: t < B (O + A); row b < B, column c < O + A <= ldq; c < O <= ldp for the actor inputs.
struct CsacPackArgs { const float* obs; const float* next; const float* act; int O, A, B; float* x_o; float* x_no; int ldp; float* xq; float* xq_pi; float* xq_next; int ldq; };
// (the bodies of the six kernels are functions over their argument struct: the kernel argument, or a member's entry of a device array
// read in place - candle_sac_group.hpp, where blockIdx.y is the member; `red` is the kernel's own 32 floats of LDS)
template <class Args>
__device__ __forceinline__ void csac_pack_body(const Args& p)
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
__global__ __launch_bounds__(256) void k_csac_pack(CsacPackArgs p) { csac_pack_body(p); }

// GaussianActor::sample then ::logp of the sampled action (util/actor.rs:196-241).  A row belongs to a group of G lanes (G a power
// of two <= 64, the smallest that holds A, chosen by the host): lane g of the group takes the columns g, g + G, ... in order, and the
// group's partial sums of logp are added by a butterfly over its G lanes - one fixed order, so the same bits run to run.
//   m the mean, l the second output (Mlp3: head2[j]; Mlp2: exp(s), s the row's own column A + j), sd = exp(clamp(l, lo, hi)),
//   u = sd z + m (train) or m (eval), a = clamp(u, amin, amax) or scale tanh(u);
//   Clamp: logp = sum_j N(a; m, sd);  Tanh: x = atanh(clamp(a / scale, +-0.999999)), logp = sum_j N(x; m, sd) - sum_j ln(1 - clamp(a)^2),
//   N(x; m, sd) = -1/2 ln 2pi - 1/2 ln sd^2 - (0.5 / sd^2)(x - m)^2.
// Gradient form (g_lpm != null): per element the TOTAL derivatives, z fixed, of logp and of a with respect to m and to the trained
// second quantity (Mlp3: head2_j; Mlp2: s, d l / d s = l), the paths through a included:
//   g_lpm = dlogp/dm, g_lpl = dlogp/d(l|s), g_am = da/dm, g_al = da/d(l|s).
// a goes into out [B][A] and into the action columns O.. of the critic input xq [B][ldq].
// Bounds: memory is touched only for b < B and j < A (lanes of rows >= B stay in the butterfly with zeros); mean row b holds
// ldm >= A (Mlp2: >= 2 A) floats; out, z, g_*: b * A + j < B * A; xq: O + j < O + A <= ldq.
struct CsacSampleArgs {
    const float* mean; int ldm; const float* head2; int mlp2; int A, B, G;
    float lo, hi; int tanh_limit; float amin, amax, scale;
    int train; uint64_t seed, counter; const float* z;
    float* out; float* xq; int ldq; int O;
    float* logp;                                       // [B]
    float* g_lpm; float* g_lpl; float* g_am; float* g_al;   // [B][A], or all null
};
// (train, counter and z are handed in beside the struct: under a group they are the member's step words, z null)
template <class Args>
__device__ __forceinline__ void csac_sample_logp_body(const Args& p, int train, uint64_t counter, const float* zrows)
{
#pragma clang fp contract(off)
    const int b = blockIdx.x * (256 / p.G) + (int)threadIdx.x / p.G;
    const int g0 = (int)threadIdx.x % p.G;
    const bool live = b < p.B;
    const float* row = p.mean + (size_t)(live ? b : 0) * p.ldm;
    float lp = 0.f, lj = 0.f;
    for (int j = g0; live && j < p.A; j += p.G) {
        const size_t t = (size_t)b * p.A + j;
        const float m = row[j];
        const float l = p.mlp2 ? expf(row[p.A + j]) : p.head2[j];
        const float sd = expf(fminf(fmaxf(l, p.lo), p.hi));
        float z = 0.f, u = m;
        if (train) {
            z = zrows ? zrows[t] : candle::randn_at(p.seed, counter, t);
            const float e = sd * z;
            u = e + m;
        }
        float a, da_du;
        if (p.tanh_limit) { const float th = tanhf(u); a = p.scale * th; da_du = p.scale * (1.0f - th * th); }
        else { a = fminf(fmaxf(u, p.amin), p.amax); da_du = (u >= p.amin && u <= p.amax) ? 1.f : 0.f; }
        p.out[t] = a;
        p.xq[(size_t)b * p.ldq + p.O + j] = a;
        // logp of a
        const float var = sd * sd;
        float x = a, dx_da = 1.f, dlj_da = 0.f;
        if (p.tanh_limit) {
            const float r = a / p.scale;
            const float tc = fminf(fmaxf(r, -0.999999f), 0.999999f);   // util.rs:268-271 atanh
            x = 0.5f * logf((1.0f + tc) / (1.0f - tc));
            dx_da = (r >= -0.999999f && r <= 0.999999f) ? 1.0f / (p.scale * (1.0f - tc * tc)) : 0.f;
            const float ac = fminf(fmaxf(a, -0.999999f), 0.999999f);   // util.rs:274-279: the action itself
            const float om = 1.0f - ac * ac;
            lj += logf(om);
            dlj_da = (a >= -0.999999f && a <= 0.999999f) ? (2.0f * ac) / om : 0.f;   // d(-ln(1 - a^2))/da
        }
        const float d = x - m;
        const float hl = 0.5f * logf(var);
        const float q = (0.5f / var) * (d * d);
        const float t0 = -0.91893853320467274178f - hl;
        lp += t0 - q;
        if (p.g_lpm) {
            const float e_m = d / var;                               // the explicit dN/dm
            const float e_sd = (d * d) / (var * sd) - 1.0f / sd;     // the explicit dN/dsd
            const float dlp_da = dlj_da - e_m * dx_da;
            const float da_dsd = train ? da_du * z : 0.f;
            const float cm = (l >= p.lo && l <= p.hi) ? 1.f : 0.f;   // the log-std clamp, closed range
            const float chain = p.mlp2 ? (sd * cm) * l : sd * cm;    // dsd / d(head2 | s)
            p.g_lpm[t] = e_m + dlp_da * da_du;
            p.g_lpl[t] = (e_sd + dlp_da * da_dsd) * chain;
            p.g_am[t] = da_du;
            p.g_al[t] = da_dsd * chain;
        }
    }
    // the group's sums: every lane of the wave takes part (groups are aligned to G lanes, xor offsets < G stay inside one)
    for (int off = p.G >> 1; off > 0; off >>= 1) { lp += __shfl_xor(lp, off); lj += __shfl_xor(lj, off); }
    if (live && g0 == 0) p.logp[b] = p.tanh_limit ? lp - lj : lp;
}
__global__ __launch_bounds__(256) void k_csac_sample_logp(CsacSampleArgs p) { csac_sample_logp_body(p, p.train, p.counter, p.z); }

// EntCoef::update (sac/ent_coef.rs:71-84) and ::alpha (:59-61).  ent: [0] log_alpha, [1] its gradient, [2] exp_avg, [3] exp_avg_sq,
// [4] alpha.  Auto: loss = mean_b(-log_alpha (logp_b + target_entropy)), so the gradient is -(1/B) sum_b (logp_b + target_entropy),
// and one AdamW step (adam_element, the dense agents' formula).  Fix: log_alpha stays.  alpha = expf(log_alpha) in both.
// One workgroup.  Bounds: b < B in row_sum; ent holds 8 floats.
struct CsacAlphaArgs { const float* logp; int B; float target_entropy; int auto_mode; AdamScalars s; float* ent; };
// (s: the AdamW scalars of this step - the struct's, or under a group the member's step words)
template <class Args>
__device__ __forceinline__ void csac_alpha_body(const Args& p, const AdamScalars& s, float* red)
{
    float sum = 0.f;
    if (p.auto_mode) sum = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
        return p.logp[b] + p.target_entropy;
    }, red);
    if (threadIdx.x != 0) return;
    float la = p.ent[0];
    if (p.auto_mode) {
        const float g = -(sum / (float)p.B);
        float m = p.ent[2], v = p.ent[3];
        adam_element(la, g, m, v, s);
        p.ent[0] = la; p.ent[1] = g; p.ent[2] = m; p.ent[3] = v;
    }
    p.ent[4] = expf(la);
}
__global__ __launch_bounds__(1024) void k_csac_alpha(CsacAlphaArgs p)
{
    __shared__ float red[32];
    csac_alpha_body(p, p.s, red);
}

// qvals_min (util/critic.rs:197-202) on (obs, a) and the output gradient of d(-q/B)/dQ_i: candle's reduce-min backward is an
// equality mask, so EVERY critic whose value equals the minimum receives the gradient (identical critics: their sum), masked by
// the output ReLU when the critic Mlp has one.  Bounds: b < B; column 0 of [B][ldq] rows.
struct CsacQminArgs { const float* q[4]; float* dq[4]; int ldq; int NC; int relu_out; float* q_min; int B; };
template <class Args>
__device__ __forceinline__ void csac_qmin_body(const Args& p)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= p.B) return;
    float mn = p.q[0][(size_t)b * p.ldq];
    for (int i = 1; i < p.NC; ++i) mn = fminf(mn, p.q[i][(size_t)b * p.ldq]);
    p.q_min[b] = mn;
    const float g = -1.0f / (float)p.B;
    for (int i = 0; i < p.NC; ++i) {
        const float qi = p.q[i][(size_t)b * p.ldq];
        p.dq[i][(size_t)b * p.ldq] = (qi == mn && !(p.relu_out && !(qi > 0.f))) ? g : 0.f;
    }
}
__global__ __launch_bounds__(256) void k_csac_qmin(CsacQminArgs p) { csac_qmin_body(p); }

// update_actor's loss and output gradient (sac/base.rs:104-122): L = mean_b(alpha logp_b - q_b).  With G_bj = sum_i d(-q/B)/da_bj
// (the critics' input gradients dxa_i, action columns, added in critic order):
//   dL/dm_bj = (alpha / B) g_lpm + G g_am,    dL/d(l|s)_bj = (alpha / B) g_lpl + G g_al.
// Grid: A + 1 workgroups.  Workgroup j < A: column j.  Mlp3: gout[b][j] = dL/dm and gh2[j] = the batch sum of dL/dhead2 in fixed
// order.  Mlp2: gout[b][j] = dL/dm, gout[b][A + j] = dL/ds.  Workgroup A: loss_actor into scal[1].
// Bounds: b < B; j < A; gout row b holds ldm >= A (Mlp2: >= 2 A) floats; dxa rows hold ldx >= O + A floats; dq_da: b * A + j < B * A.
struct CsacActorArgs {
    const float* dxa[4]; int ldx; int NC; int O, A, B; int mlp2;
    const float* g_lpm; const float* g_lpl; const float* g_am; const float* g_al;
    const float* ent; const float* logp; const float* q_min;
    float* gout; int ldm; float* gh2; float* dq_da;
    float* scal; int accumulate;
};
template <class Args>
__device__ __forceinline__ void csac_actor_grad_body(const Args& p, float* red)
{
    const float invB = 1.0f / (float)p.B;
    const float alpha = p.ent[4];
    const int j = blockIdx.x;
    if (j < p.A) {
        const float s = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
            const size_t t = (size_t)b * p.A + j;
            float G = p.dxa[0][(size_t)b * p.ldx + p.O + j];
            for (int i = 1; i < p.NC; ++i) G += p.dxa[i][(size_t)b * p.ldx + p.O + j];
            p.dq_da[t] = -(G * (float)p.B);
            const float ab = alpha * invB;
            const float gm = ab * p.g_lpm[t] + G * p.g_am[t];
            const float gl = ab * p.g_lpl[t] + G * p.g_al[t];
            p.gout[(size_t)b * p.ldm + j] = gm;
            if (p.mlp2) p.gout[(size_t)b * p.ldm + p.A + j] = gl;
            return gl;
        }, red);
        if (!p.mlp2 && threadIdx.x == 0) p.gh2[j] = s;
        return;
    }
    const float s = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
        const float al = alpha * p.logp[b];
        return al - p.q_min[b];
    }, red);
    if (threadIdx.x == 0) p.scal[1] = candle::acc(p.accumulate ? p.scal[1] : 0.f, s, invB);
}
__global__ __launch_bounds__(1024) void k_csac_actor_grad(CsacActorArgs p)
{
    __shared__ float red[32];
    csac_actor_grad_body(p, red);
}

// update_critic (sac/base.rs:63-102): next_q = min_i Qtgt_i(next_obs, next_a) - alpha next_logp, tgt = r + gamma_not_done next_q with
// gamma_not_done = (1 - is_terminated) gamma in f32 (is_truncated ignored); loss = mean_i mean_b loss(Q_i - tgt), MSE or smooth L1
// (util.rs:144-152); dL/dQ_i = loss'(Q_i - tgt) / (NC B), masked by the output ReLU when the critic Mlp has one.
// scal[0] loss_critic (summed over the updates of one opt), scal[2] alpha.  One workgroup.  Bounds: b < B; column 0 of [B][ldq] rows.
struct CsacCriticArgs {
    const float* q[4]; float* dq[4]; const float* qt[4]; int ldq; int NC; int relu_out;
    const float* reward; const int8_t* term; float gamma; const float* ent; const float* next_logp;
    float* tgt; int loss_kind; float* scal; int accumulate; int B;
};
template <class Args>
__device__ __forceinline__ void csac_critic_loss_body(const Args& p, float* red)
{
    const float invB = 1.0f / (float)p.B, invNC = 1.0f / (float)p.NC;
    const float alpha = p.ent[4];
    float total = 0.f;
    for (int i = 0; i < p.NC; ++i) {   // critic by critic, summed in critic order (Tensor::stack(..).mean_all())
        const float si = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
            float nq = p.qt[0][(size_t)b * p.ldq];
            for (int k = 1; k < p.NC; ++k) nq = fminf(nq, p.qt[k][(size_t)b * p.ldq]);
            const float ent = alpha * p.next_logp[b];
            nq = nq - ent;
            const float gnd = (1.0f - (float)p.term[b]) * p.gamma;
            const float c = gnd * nq;
            const float t = p.reward[b] + c;
            if (i == 0) p.tgt[b] = t;
            const float q = p.q[i][(size_t)b * p.ldq];
            const float d = q - t;
            float l, g;
            candle::critic_loss_elem(p.loss_kind, d, l, g);
            float gq = (g * invB) * invNC;
            if (p.relu_out && !(q > 0.f)) gq = 0.f;
            p.dq[i][(size_t)b * p.ldq] = gq;
            return l;
        }, red);
        total = candle::acc(total, si, invB);
    }
    if (threadIdx.x == 0) {
        p.scal[0] = (p.accumulate ? p.scal[0] : 0.f) + total * invNC;
        p.scal[2] = alpha;
    }
}
__global__ __launch_bounds__(1024) void k_csac_critic_loss(CsacCriticArgs p)
{
    __shared__ float red[32];
    csac_critic_loss_body(p, red);
}

}  // namespace


// ================================================================================================
// The actor, the critics and their steps, Policy::sample, the parameter views and the checkpoints are CandleAgent's
// (candle_actor.hpp); SAC adds its update schedule, the entropy coefficient and the critics' input-gradient chain.
struct CandleSac : CandleAgent<CandleSac, bdr_candle_sac_config> {
    static constexpr const char* NAME = "SAC (candle)";
    static constexpr int N_RECORD = 3;   // scal: loss_critic and loss_actor summed over the updates of one opt, alpha
    // batch buffers
    float *xq_pi = nullptr, *xq_next = nullptr;               // critic inputs (obs | a), (next_obs | next_a)
    std::vector<float*> pn_act;                               // the updated actor on next_obs
    std::vector<float*> cp_act[4], cp_dy[4];                  // critics on (obs, a), the gradients of their input-gradient chain
    float* dxa[4] = {nullptr};                                // d(-q/B)/d(obs | a) per critic, [B][Kq]
    float *g_lpm = nullptr, *g_lpl = nullptr, *g_am = nullptr, *g_al = nullptr;   // k_csac_sample_logp's partials [B][A]
    float *pr_a = nullptr, *pr_next_a = nullptr, *pr_dqda = nullptr;              // [B][A]
    float *pr_qmin = nullptr, *pr_nlogp = nullptr;            // [B] (logp: pr_logp, tgt: pr_tgt)
    float* u_z = nullptr;                                     // host noise rows of update_on_batch: z_pi | z_next
    float* ent = nullptr;                                     // log_alpha, grad, exp_avg, exp_avg_sq, alpha (k_csac_alpha)
    uint64_t step_al = 0;

    int32_t alloc_batch(int Bn)
    {
        for (auto p : {&xq_pi, &xq_next}) BDR_TRY(alloc(p, (size_t)Bn * qn.L[0].Kp, BATCH));
        BDR_TRY(layer_bufs(pn, Bn, pn_act));
        for (int i = 0; i < NC; ++i) {
            BDR_TRY(layer_bufs(qn, Bn, cp_act[i])); BDR_TRY(layer_bufs(qn, Bn, cp_dy[i]));
            BDR_TRY(alloc(&dxa[i], (size_t)Bn * qn.L[0].Kp, BATCH));
        }
        for (auto p : {&g_lpm, &g_lpl, &g_am, &g_al, &pr_a, &pr_next_a, &pr_dqda}) BDR_TRY(alloc(p, (size_t)Bn * A, BATCH));
        for (auto p : {&pr_qmin, &pr_nlogp}) BDR_TRY(alloc(p, Bn, BATCH));
        return BDR_OK;
    }
    int32_t alloc_staging(uint64_t n) { return alloc(&u_z, 2 * n * A, STAGING, false); }
    // the entropy block as one arena: log_alpha, its gradient and moments, and alpha - the copy params_written derives, with the bits
    // the source's k_csac_alpha wrote
    void own_arenas(std::vector<StateArena>& out) { out.push_back({ent, 8}); }
    void own_steps(const CandleSac& s) { step_al = s.step_al; }
    double* own_hyper(int32_t id)
    {
        if (cfg.ent_coef_mode != BDR_ENT_COEF_AUTO) return nullptr;
        return id == BDR_HYPER_ENT_COEF_LR ? &cfg.ent_coef_lr : id == BDR_HYPER_TARGET_ENTROPY ? &cfg.target_entropy : nullptr;
    }
    int32_t init_own()
    {
        BDR_TRY(alloc(&ent, 8, AGENT));
        // ent_coef.rs:36-48: Fix(alpha): Init::Const(alpha.ln()); Auto: Init::Const(0.0)
        const float la = cfg.ent_coef_mode == BDR_ENT_COEF_AUTO ? 0.f : (float)std::log(cfg.ent_coef_alpha);
        const float h[8] = {la, 0.f, 0.f, 0.f, expf(la), 0.f, 0.f, 0.f};
        BDR_HIP(hipMemcpyAsync(ent, h, sizeof h, hipMemcpyHostToDevice, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        return BDR_OK;
    }

    // actor.sample and actor.logp of Bn rows from the actor's last layer; grads: also the partials of update_actor
    int32_t sample_logp(const float* last, int Bn, const float* z, float* out, float* xqd, float* logp, bool grads, const char* name)
    {
        const SampleElem e = sample_elem(Bn, z);   // the operands, and the draws this call takes from the stream
        CsacSampleArgs p{};
        p.mean = last; p.ldm = pn.L.back().Np; p.head2 = e.head2; p.mlp2 = e.mlp2; p.A = A; p.B = Bn;
        p.lo = e.lo; p.hi = e.hi; p.tanh_limit = e.tanh_limit; p.amin = e.amin; p.amax = e.amax; p.scale = e.scale;
        p.train = e.train; p.seed = e.seed; p.counter = e.counter; p.z = e.z;
        p.out = out; p.xq = xqd; p.ldq = qn.L[0].Kp; p.O = O; p.logp = logp;
        if (grads) { p.g_lpm = g_lpm; p.g_lpl = g_lpl; p.g_am = g_am; p.g_al = g_al; }
        p.G = 1;
        while (p.G < A && p.G < 64) p.G *= 2;   // lanes per row
        const int rows = 256 / p.G;             // rows per workgroup
        Bracket br(this, name);
        BDR_HIP(step_launch(stream, true, k_csac_sample_logp, dim3((Bn + rows - 1) / rows), dim3(256), p));
        return BDR_OK;
    }

    // One iteration of the Sac::opt_ loop on device-resident rows (f32 obs / next_obs / act).  z_pi / z_next: device N(0,1) rows or null.
    int32_t update(int Bn, const float* obs, const float* act, const float* next_obs, const float* reward, const int8_t* term,
                   const int8_t* /*trunc*/, bool first, const float* z_pi = nullptr, const float* z_next = nullptr)
    {
        BDR_TRY(ensure_batch(Bn));
        const int Lq = (int)qn.L.size(), Lp = (int)pn.L.size();
        const int ldq = qn.L[Lq - 1].Np;
        {
            CsacPackArgs p{obs, next_obs, act, O, A, Bn, x_o, x_no, pn.L[0].Kp, xq, xq_pi, xq_next, qn.L[0].Kp};
            const size_t n = (size_t)Bn * (O + A);
            Bracket br(this, "pack");
            BDR_HIP(step_launch(stream, true, k_csac_pack, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), p));
        }
        // ---------------- update_actor (:104-122) ----------------
        BDR_TRY(actor_forward(x_o, p_act, Bn));
        BDR_TRY(sample_logp(p_act[Lp - 1], Bn, z_pi, pr_a, xq_pi, pr_logp, true, "csac_sample_logp"));
        {   // EntCoef::update(logp.detach()) before alpha is read (:111)
            CsacAlphaArgs p{};
            p.logp = pr_logp; p.B = Bn; p.target_entropy = (float)cfg.target_entropy; p.auto_mode = cfg.ent_coef_mode == BDR_ENT_COEF_AUTO ? 1 : 0;
            if (p.auto_mode) { step_al += 1; p.s = adam_scalars_for(true, cfg.ent_coef_lr, 0.9, 0.999, 1e-8, 0.01, step_al); }   // candle-nn ParamsAdamW::default()
            p.ent = ent;
            Bracket br(this, "csac_alpha");
            BDR_HIP(step_launch(stream, false, k_csac_alpha, dim3(1), dim3(1024), p));
        }
        // the online critics on (obs, act) and (obs, a): 2 NC pairs.  No critic parameter changes before update_critic, so the
        // (obs, act) activations are also that step's predictions and activations.
        {
            const float* params[8]; const float* x[8]; std::vector<float*>* acts[8];
            for (int i = 0; i < NC; ++i) { params[i] = q_p[i]; x[i] = xq; acts[i] = &c_act[i]; params[NC + i] = q_p[i]; x[NC + i] = xq_pi; acts[NC + i] = &cp_act[i]; }
            BDR_TRY(mlp_forward(qn, 2 * NC, params, x, acts, Bn, "q_fwd"));
        }
        {
            CsacQminArgs p{};
            for (int i = 0; i < NC; ++i) { p.q[i] = cp_act[i][Lq - 1]; p.dq[i] = cp_dy[i][Lq - 1]; }
            p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu; p.q_min = pr_qmin; p.B = Bn;
            Bracket br(this, "csac_qmin");
            BDR_HIP(step_launch(stream, false, k_csac_qmin, dim3((Bn + 255) / 256), dim3(256), p));
        }
        // dq/da: the critics' input gradients, layer by layer for all NC, the input layer without a mask
        for (int l = Lq - 1; l >= 0; --l) {
            const float* pb[4]; const float* dy[4]; float* dx[4]; const float* mask[4];
            for (int i = 0; i < NC; ++i) { pb[i] = q_p[i]; dy[i] = cp_dy[i][l]; dx[i] = l ? cp_dy[i][l - 1] : dxa[i]; mask[i] = l ? cp_act[i][l - 1] : nullptr; }
            Bracket br(this, "q_dx");
            BDR_TRY(dense_dx_z(stream, qn.L[l], NC, pb, dy, dx, l ? mask : nullptr, Bn, true));
        }
        {
            CsacActorArgs p{};
            for (int i = 0; i < NC; ++i) p.dxa[i] = dxa[i];
            p.ldx = qn.L[0].Kp; p.NC = NC; p.O = O; p.A = A; p.B = Bn; p.mlp2 = mlp2() ? 1 : 0;
            p.g_lpm = g_lpm; p.g_lpl = g_lpl; p.g_am = g_am; p.g_al = g_al; p.ent = ent; p.logp = pr_logp; p.q_min = pr_qmin;
            p.gout = p_dy[Lp - 1]; p.ldm = pn.L[Lp - 1].Np; p.gh2 = h2_part; p.dq_da = pr_dqda;
            p.scal = scal; p.accumulate = first ? 0 : 1;
            Bracket br(this, "csac_actor_grad");
            BDR_HIP(step_launch(stream, false, k_csac_actor_grad, dim3(A + 1), dim3(1024), p));
        }
        BDR_TRY(actor_step(Bn));
        // ---------------- update_critic (:63-102) ----------------
        // next_a, next_logp from the UPDATED actor (:77-78)
        BDR_TRY(actor_forward(x_no, pn_act, Bn));
        BDR_TRY(sample_logp(pn_act[Lp - 1], Bn, z_next, pr_next_a, xq_next, pr_nlogp, false, "csac_sample_logp"));
        {
            const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
            for (int i = 0; i < NC; ++i) { params[i] = q_t[i]; x[i] = xq_next; acts[i] = &t_act[i]; }
            BDR_TRY(mlp_forward(qn, NC, params, x, acts, Bn, "q_tgt_fwd"));
        }
        {
            CsacCriticArgs p{};
            for (int i = 0; i < NC; ++i) { p.q[i] = c_act[i][Lq - 1]; p.dq[i] = c_dy[i][Lq - 1]; p.qt[i] = t_act[i][Lq - 1]; }
            p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu;
            p.reward = reward; p.term = term; p.gamma = (float)cfg.gamma; p.ent = ent; p.next_logp = pr_nlogp; p.tgt = pr_tgt;
            p.loss_kind = cfg.critic_loss; p.scal = scal; p.accumulate = first ? 0 : 1; p.B = Bn;
            Bracket br(this, "csac_critic_loss");
            BDR_HIP(step_launch(stream, false, k_csac_critic_loss, dim3(1), dim3(1024), p));
        }
        BDR_TRY(critic_step(Bn));
        n_opts += 1;
        last_B = Bn;
        return BDR_OK;
    }

    const char* kind() const override { return "candle_sac"; }
    void record_keys(std::vector<std::string>& keys) override { keys = {"loss_critic", "loss_actor", "ent_coef"}; }
    int32_t record(float* out, int cap, int* n) override
    {
        float h[3];
        BDR_HIP(hipMemcpyAsync(h, scal, 12, hipMemcpyDeviceToHost, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        if (cap < 3) return fail(BDR_ERR_INVALID, "SAC record needs 3 slots");
        // sac/base.rs:136-146: the two losses divided by n_updates_per_opt; ent_coef = alpha after the last update
        const float nu = (float)cfg.n_updates_per_opt;
        out[0] = h[0] / nu; out[1] = h[1] / nu; out[2] = h[2];
        *n = 3;
        return BDR_OK;
    }

    // ---- log_alpha: model 1 + 2 NC (value, +100 grad, +200 exp_avg, +300 exp_avg_sq), one float each of `ent` ----
    bool own_view(int k, int role, ParamView* pv)
    {
        if (k == 0) *pv = {ent + role, 1, 1, [](const float* in, float* ref) { ref[0] = in[0]; }, [](const float* ref, float* in) { in[0] = ref[0]; }};
        return k == 0;
    }
    int32_t params_written(int which) override   // a new log_alpha: alpha = exp(log_alpha) is what the loss kernels read
    {
        if (which != 1 + 2 * NC) return BDR_OK;
        float la = 0.f;
        BDR_TRY(arena_to_host(ent, &la, 1));
        const float al = expf(la);
        return arena_from_host(ent + 4, &al, 1);
    }
    void own_files(std::vector<CheckpointFile>& files)   // sac/base.rs:244-270: the core's three files and ent_coef.pt with log_alpha [1]
    {
        files.push_back({"ent_coef", {{"log_alpha", {1}}}, {1 + 2 * NC}, {1 + 2 * NC}});
    }
};

namespace {
constexpr const char* kOneRow =
    "SAC needs at least 2 rows per batch: at one row the reference squeezes the TD target to a scalar while each prediction keeps "
    "shape [1], and candle's same-shape tensor ops reject that pair (sac/base.rs:83, util/critic.rs:205-218)";
}  // namespace

extern "C" {

void bdr_candle_sac_config_default(bdr_candle_sac_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    // sac/config.rs:82-93
    c->gamma = 0.99; c->ent_coef_mode = BDR_ENT_COEF_FIX; c->ent_coef_alpha = 1.0; c->n_updates_per_opt = 1; c->batch_size = 1;
    c->critic_loss = BDR_LOSS_MSE; c->device = -1; c->train = 0;
    c->target_entropy = 0.0; c->ent_coef_lr = 3e-4;   // read in Auto mode only, which has no default of its own
    c->actor_kind = BDR_ACTOR_MLP3;
    // MultiCriticConfig (util/critic.rs:35-43), GaussianActorConfig (util/actor.rs:44-55)
    c->n_critics = 2; c->critic_tau = 0.005;
    c->lr_actor = c->lr_critic = 3e-4;
    c->min_log_std = -20.0; c->max_log_std = 2.0;
    c->action_limit = BDR_ACTION_LIMIT_CLAMP; c->action_min = -1.0; c->action_max = 1.0; c->action_scale = 1.0;
    for (bdr_adamw_config* o : {&c->opt_actor, &c->opt_critic}) { o->opt_kind = BDR_OPT_ADAM; o->beta1 = 0.9; o->beta2 = 0.999; o->weight_decay = 0.01; o->eps = 1e-8; }
    for (bdr_mlp_config* m : {&c->actor, &c->critic}) m->activation_out = BDR_ACTIVATION_NONE;
}

int32_t bdr_candle_sac_create(const bdr_candle_sac_config* cfg, bdr_agent** out)
{
    BDR_REQUIRE(cfg && out, "null argument");
    BDR_REQUIRE(cfg->ent_coef_mode == BDR_ENT_COEF_FIX || cfg->ent_coef_mode == BDR_ENT_COEF_AUTO, "unknown ent_coef_mode %d", cfg->ent_coef_mode);
    BDR_REQUIRE(cfg->ent_coef_mode == BDR_ENT_COEF_AUTO || cfg->ent_coef_alpha > 0.0, "Fix(alpha) needs alpha > 0 (log_alpha = ln(alpha))");
    return CandleSac::create(*cfg, out, nullptr, nullptr, kOneRow, cfg->actor_kind);
}

int32_t bdr_candle_sac_update_on_batch(bdr_agent* base, uint64_t n, const float* obs, const float* act, const float* next_obs,
                                       const float* reward, const int8_t* term, const int8_t* trunc, const float* z_pi, const float* z_next, float* rec3)
{
    BDR_REQUIRE(base && obs && act && next_obs && reward && term && trunc, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "candle_sac"), "not a candle SAC agent");
    BDR_REQUIRE(n != 1, "%s", kOneRow);
    BDR_REQUIRE(n >= 2 && n <= 65536, "batch size out of range");
    CandleSac* a = static_cast<CandleSac*>(base);
    BDR_TRY(a->stage_batch(n, obs, act, next_obs, reward, term, trunc));
    float* dz_pi = nullptr; float* dz_next = nullptr;
    if (z_pi) { dz_pi = a->u_z; BDR_HIP(hipMemcpyAsync(dz_pi, z_pi, n * a->A * 4, hipMemcpyHostToDevice, a->stream)); }
    if (z_next) { dz_next = a->u_z + n * a->A; BDR_HIP(hipMemcpyAsync(dz_next, z_next, n * a->A * 4, hipMemcpyHostToDevice, a->stream)); }
    BDR_TRY(a->update((int)n, a->u_obs, a->u_act, a->u_next, a->u_rew, a->u_term, a->u_trunc, true, dz_pi, dz_next));
    return a->batch_done(rec3);
}

// Parity probes of the LAST update (see include/border_amd.h)
int32_t bdr_candle_sac_probe(bdr_agent* base, int32_t what, float* out, uint64_t n)
{
    BDR_REQUIRE(base && out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "candle_sac"), "not a candle SAC agent");
    CandleSac* a = static_cast<CandleSac*>(base);
    BDR_HIP(hipSetDevice(a->device));
    const int Bn = a->last_B, NC = a->NC;
    BDR_REQUIRE(Bn > 0, "no update has run yet");
    BDR_HIP(hipStreamSynchronize(a->stream));
    if (what < 0 || what > 7) return fail(BDR_ERR_INVALID, "unknown SAC probe %d", what);
    if (what == 6) {   // Q_i(obs, act): column 0 of the critics' last layer
        BDR_REQUIRE(n == (uint64_t)NC * Bn, "q_pred holds n_critics x batch values");
        const int Lq = (int)a->qn.L.size(), ld = a->qn.L[Lq - 1].Np;
        std::vector<float> h((size_t)Bn * ld);
        for (int i = 0; i < NC; ++i) {
            BDR_HIP(hipMemcpy(h.data(), a->c_act[i][Lq - 1], h.size() * 4, hipMemcpyDeviceToHost));
            for (int b = 0; b < Bn; ++b) out[(size_t)i * Bn + b] = h[(size_t)b * ld];
        }
        return BDR_OK;
    }
    if (what == 0 || what == 3 || what == 7) {
        BDR_REQUIRE(n == (uint64_t)Bn * a->A, "this probe holds batch x act_dim values");
        BDR_HIP(hipMemcpy(out, what == 0 ? a->pr_a : what == 3 ? a->pr_next_a : a->pr_dqda, n * 4, hipMemcpyDeviceToHost));
        return BDR_OK;
    }
    const float* rows[6] = {nullptr, a->pr_logp, a->pr_qmin, nullptr, a->pr_nlogp, a->pr_tgt};
    BDR_REQUIRE(n == (uint64_t)Bn, "this probe holds batch values");
    BDR_HIP(hipMemcpy(out, rows[what], (size_t)Bn * 4, hipMemcpyDeviceToHost));
    return BDR_OK;
}

// Policy::sample (util/actor.rs:226-241); out: [n][act_dim]
int32_t bdr_candle_sac_sample(bdr_agent* base, uint64_t n, const float* obs, float* act_out)
{
    BDR_REQUIRE(base && obs && act_out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "candle_sac"), "not a candle SAC agent");
    return static_cast<CandleSac*>(base)->sample(n, obs, act_out);
}

int32_t bdr_candle_sac_sample_device(bdr_agent* base, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out)
{
    BDR_REQUIRE(base && obs_dev && act_out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "candle_sac"), "not a candle SAC agent");
    return static_cast<CandleSac*>(base)->sample_device(n, obs_dev, row_stride, act_out);
}

}  // extern "C"

// the launch grouping of candle SAC agents (bdr_candle_sac_group_*): it needs CandleSac and the kernel bodies above
#include "candle_sac_group.hpp"
