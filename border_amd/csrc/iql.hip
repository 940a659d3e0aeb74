// IQL agent on MI355X: Iql::opt_ (border-candle-agent/src/iql/base.rs:157-188) with update_value (:75-86), update_critic (:88-121)
// and update_actor (:123-155); value = Mlp (iql/value.rs, mlp.rs:14-24), critics = MultiCritic of Mlp on cat(obs, act)
// (util/critic.rs), actor = GaussianActor (util/actor.rs) over Mlp3 (mlp/mlp3.rs).
// Dense layers run on the FP32-MFMA kernels of dense.hpp (unchanged); the IQL math - expectile loss, TD target from the value
// network, advantage weights, Gaussian log-likelihood - and its hand-derived backward are the kernels below.  Every batch-wide sum
// is formed in one fixed order (rows in blocks of 32, a 32-lane butterfly per block, the block partials added in block order), so an
// update gives the same bits run to run.  Reference quirks kept on purpose:
//   gamma_not_done counts is_truncated (util.rs:235-255); the Tanh limit's log-Jacobian uses the action itself, not action / scale
//   (util/actor.rs:210-218, util.rs:274-279); MultiCritic::save writes the ONLINE critics into critic.tgt.pt and load reads both
//   files into the online critics, leaving the targets alone (util/critic.rs:272-298).
#include <algorithm>
#include <cstdlib>

#include "candle_actor.hpp"
#include "dense.hpp"

using namespace bdr;

int32_t bdr_iql_sample(bdr_agent* base, uint64_t n, const float* obs, float* act_out);

namespace {

__global__ void k_iql_randn(float* __restrict__ out, size_t n, uint64_t seed, uint64_t counter)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = candle::randn_at(seed, counter, i);
}

// obs / next_obs / act rows -> the zero-padded inputs of the value + actor ([B][Kp], obs and next_obs) and of the critics ([B][Kq], obs | act)
struct IqlPackArgs { const float* obs; const float* next; const float* act; int O, A, B; float* x_o; float* x_no; int ldp; float* xq; int ldq; };
__global__ __launch_bounds__(256) void k_iql_pack(IqlPackArgs p)
{
    const int W = p.O + p.A;
    const size_t n = (size_t)p.B * W;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) {
        const int b = (int)(t / W), c = (int)(t % W);
        if (c < p.O) {
            const float o = p.obs[(size_t)b * p.O + c];
            p.x_o[(size_t)b * p.ldp + c] = o;
            p.x_no[(size_t)b * p.ldp + c] = p.next[(size_t)b * p.O + c];
            p.xq[(size_t)b * p.ldq + c] = o;
        } else {
            p.xq[(size_t)b * p.ldq + c] = p.act[(size_t)b * p.A + (c - p.O)];
        }
    }
}

// (a) update_value (iql/base.rs:75-86): q = min_i Qtgt_i(obs, act), u = q - V(obs), loss = mean(|tau - 1[u < 0]| u^2) (util.rs:262-266),
// dL/dV = -2 |tau - 1[u < 0]| u / B (masked by the output ReLU when the value Mlp has one).  Column 0 of dv only: the padding columns
// are zero from allocation and nothing else stores there.
struct IqlValueArgs {
    const float* qt[4]; int ldq; int NC;
    const float* v; float* dv; int ldv; int relu_out;
    float tau;
    float* q_min; float* v_out; float* u_out;   // probes [B]
    float* loss; int accumulate; int B;
};
__global__ __launch_bounds__(1024) void k_iql_value_loss(IqlValueArgs p)
{
    __shared__ float red[32];
    const float invB = 1.0f / (float)p.B;
    const float s = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
        float qm = p.qt[0][(size_t)b * p.ldq];
        for (int i = 1; i < p.NC; ++i) qm = fminf(qm, p.qt[i][(size_t)b * p.ldq]);
        const float v = p.v[(size_t)b * p.ldv];
        const float u = qm - v;
        const float wt = fabsf(p.tau - (u < 0.f ? 1.0f : 0.0f));
        const float uu = u * u;
        const float l = wt * uu;
        const float g2 = -2.0f * wt;
        float g = g2 * u * invB;
        if (p.relu_out && !(v > 0.f)) g = 0.f;
        p.dv[(size_t)b * p.ldv] = g;
        p.q_min[b] = qm; p.v_out[b] = v; p.u_out[b] = u;
        return l;
    }, red);
    if (threadIdx.x == 0) p.loss[0] = candle::acc(p.accumulate ? p.loss[0] : 0.f, s, invB);
}

// (b) update_critic (iql/base.rs:88-121): tgt = r + gamma_not_done * V'(next_obs), gamma_not_done = (1 - (term | trunc)) * gamma in f32
// (util.rs:235-255); loss = mean_i mean_b loss(Q_i - tgt), MSE or smooth L1 (util.rs:144-152); dL/dQ_i = loss'(Q_i - tgt) / (NC * B)
struct IqlCriticArgs {
    const float* q[4]; float* dq[4]; int ldq; int NC; int relu_out;
    const float* vn; int ldv;
    const float* reward; const int8_t* term; const int8_t* trunc; float gamma;
    float* tgt; float* v_next;   // [B]
    int loss_kind; float* loss; int accumulate; int B;
};
__global__ __launch_bounds__(1024) void k_iql_critic_loss(IqlCriticArgs p)
{
    __shared__ float red[32];
    for (int b = threadIdx.x; b < p.B; b += 1024) {
#pragma clang fp contract(off)
        const float vn = p.vn[(size_t)b * p.ldv];
        const float done = (float)(p.term[b] | p.trunc[b]);
        const float gnd = (1.0f - done) * p.gamma;
        const float c = gnd * vn;
        p.tgt[b] = p.reward[b] + c;
        p.v_next[b] = vn;
    }
    const float scale = 1.0f / ((float)p.B * (float)p.NC);
    float total = p.accumulate ? p.loss[0] : 0.f;
    for (int i = 0; i < p.NC; ++i) {   // critic by critic; a thread reads back only the targets it wrote itself
        const float si = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
            const float q = p.q[i][(size_t)b * p.ldq];
            const float d = q - p.tgt[b];
            float l, g;
            if (p.loss_kind == 1) { const float z = fabsf(d); const float hz = 0.5f * z; l = z < 1.f ? hz * z : z - 0.5f; g = z < 1.f ? d : (d > 0.f ? 1.f : -1.f); }
            else { l = d * d; g = 2.f * d; }
            float gq = g * scale;
            if (p.relu_out && !(q > 0.f)) gq = 0.f;
            p.dq[i][(size_t)b * p.ldq] = gq;
            return l;
        }, red);
        total = candle::acc(total, si, scale);
    }
    if (threadIdx.x == 0) p.loss[0] = total;
}

// (c) + (d) update_actor (iql/base.rs:123-155): adv = min_i Qtgt_i(obs, act) - V'(obs); w = clamp(exp(inv_lambda adv), 0, exp_adv_max) or
// softmax(inv_lambda adv) over the batch (one batch-wide max and sum); logp of the batch actions under N(mean, std^2), std =
// exp(clamp(head2, min, max)) (util/actor.rs:196-223, normal_logp :19-25; Tanh limit: x = atanh(clamp(a / scale)) plus the log-Jacobian
// of `a`); loss = mean(-logp w).  Gradients: dL/dmean = -(w/B) (x - mean) / var and dL/dhead2_j = sum_b -(w_b/B)(-1 + (x - mean)^2 / var)
// where min <= head2_j <= max (0 outside: the clamp).
struct IqlActorArgs {
    const float* qt[4]; int ldq; int NC;
    const float* vo; int ldv;
    const float* mean; int ldm; const float* head2; const float* act; int A;
    float lo, hi; int tanh_limit; float scale;
    float inv_lambda, exp_adv_max; int softmax;
    float* q_min; float* w; float* logp;   // [B]
    float* gmean; float* gh2;              // [B][ldm], [A]
    float* loss; int accumulate; int B;
};
__device__ __forceinline__ float iql_x(const IqlActorArgs& p, float a)
{
#pragma clang fp contract(off)
    if (!p.tanh_limit) return a;
    const float t = fminf(fmaxf(a / p.scale, -0.999999f), 0.999999f);   // util.rs:268-271 atanh
    const float r = (1.0f + t) / (1.0f - t);
    return 0.5f * logf(r);
}
__global__ __launch_bounds__(1024) void k_iql_actor_loss(IqlActorArgs p)
{
    __shared__ float red[32];
    const float invB = 1.0f / (float)p.B;
    for (int b = threadIdx.x; b < p.B; b += 1024) {
#pragma clang fp contract(off)
        float qm = p.qt[0][(size_t)b * p.ldq];
        for (int i = 1; i < p.NC; ++i) qm = fminf(qm, p.qt[i][(size_t)b * p.ldq]);
        const float adv = qm - p.vo[(size_t)b * p.ldv];
        const float z = adv * p.inv_lambda;
        p.q_min[b] = qm;
        p.w[b] = p.softmax ? z : fminf(fmaxf(expf(z), 0.0f), p.exp_adv_max);
    }
    if (p.softmax) {   // softmax(z, 0): exp(z - max) / sum(exp(z - max))
        const float mx = candle::row_max(p.B, [&](int b) { return p.w[b]; }, red);
        const float s = candle::row_sum(p.B, [&](int b) { const float e = expf(p.w[b] - mx); p.w[b] = e; return e; }, red);
        for (int b = threadIdx.x; b < p.B; b += 1024) p.w[b] = p.w[b] / s;
    }
    // per row: logp and dL/dmean
    const float s_wl = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
        const float wb = p.w[b];
        const float gl = -wb * invB;   // dL/dlogp_b
        float lp = 0.f, lj = 0.f;
        for (int j = 0; j < p.A; ++j) {
            const float ls = fminf(fmaxf(p.head2[j], p.lo), p.hi);
            const float sd = expf(ls);
            const float var = sd * sd;
            const float a = p.act[(size_t)b * p.A + j];
            const float x = iql_x(p, a);
            const float mu = p.mean[(size_t)b * p.ldm + j];
            const float d = x - mu;
            const float hl = 0.5f * logf(var);
            const float q = (0.5f / var) * (d * d);
            const float t0 = -0.91893853320467274178f - hl;
            lp += t0 - q;
            if (p.tanh_limit) { const float ac = fminf(fmaxf(a, -0.999999f), 0.999999f); lj += logf(1.0f - ac * ac); }
            p.gmean[(size_t)b * p.ldm + j] = gl * (d / var);
        }
        const float l = p.tanh_limit ? lp - lj : lp;
        p.logp[b] = l;
        return wb * l;
    }, red);
    if (threadIdx.x == 0) p.loss[0] = candle::acc(p.accumulate ? p.loss[0] : 0.f, -s_wl, invB);
    // dL/dhead2_j: one fixed-order batch sum per action dimension
    for (int j = 0; j < p.A; ++j) {
        const float h = p.head2[j];
        const float ls = fminf(fmaxf(h, p.lo), p.hi);
        const float sd = expf(ls);
        const float var = sd * sd;
        const float s = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
            const float d = iql_x(p, p.act[(size_t)b * p.A + j]) - p.mean[(size_t)b * p.ldm + j];
            const float r = (d * d) / var - 1.0f;
            return -(p.w[b] * invB) * r;
        }, red);
        if (threadIdx.x == 0) p.gh2[j] = (h >= p.lo && h <= p.hi) ? s : 0.f;
    }
}

// Policy::sample (util/actor.rs:226-241): train: mean + std z, eval: mean; then clamp or scale * tanh.  out [n][A]
struct IqlSampleArgs {
    const float* mean; int ldm; const float* head2; int A, n;
    float lo, hi; int tanh_limit; float amin, amax, scale;
    int train; uint64_t seed, counter;
    float* out;
};
__global__ __launch_bounds__(256) void k_iql_sample(IqlSampleArgs p)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.n * p.A) return;
    const int b = t / p.A, j = t % p.A;
    float a = p.mean[(size_t)b * p.ldm + j];
    if (p.train) {
        const float sd = expf(fminf(fmaxf(p.head2[j], p.lo), p.hi));
        const float e = sd * candle::randn_at(p.seed, p.counter, (size_t)t);
        a = e + a;
    }
    if (p.tanh_limit) { const float th = tanhf(a); a = p.scale * th; }
    else a = fminf(fmaxf(a, p.amin), p.amax);
    p.out[t] = a;
}

}  // namespace

// ================================================================================================
struct Iql : bdr_agent {
    bdr_iql_config cfg;
    int O = 0, A = 0, NC = 2;
    MlpLayout vn, pn, qn;          // value, actor mean (head2 follows pn in the actor arena), critic
    size_t h2_off = 0, pi_total = 0;   // head2 at h2_off (= pn.total) in the actor arena; pi_total = pn.total + pad64(A)
    // arenas: parameters, gradients, exp_avg, exp_avg_sq
    float *pi_p = nullptr, *pi_g = nullptr, *pi_m = nullptr, *pi_v = nullptr;
    float *v_p = nullptr, *v_g = nullptr, *v_m = nullptr, *v_v = nullptr;
    float* q_p[4] = {nullptr}; float* q_t[4] = {nullptr}; float* q_g[4] = {nullptr}; float* q_m[4] = {nullptr}; float* q_v[4] = {nullptr};
    uint64_t step_pi = 0, step_v = 0, step_q = 0;
    // batch buffers
    int B = 0;
    float *x_o = nullptr, *x_no = nullptr, *xq = nullptr;
    std::vector<float*> v_act, vo_act, vn_act, v_dy;          // V(obs) (step 1), V'(obs), V'(next_obs); value gradients
    std::vector<float*> p_act, p_dy;                          // actor
    std::vector<float*> c_act[4], t_act[4], c_dy[4];          // online critics on (obs, act), target critics, critic gradients
    float *pr_qmin1 = nullptr, *pr_v = nullptr, *pr_u = nullptr, *pr_tgt = nullptr, *pr_qmin3 = nullptr, *pr_w = nullptr, *pr_logp = nullptr, *pr_vnext = nullptr;
    float *v_part = nullptr, *pi_part = nullptr, *q_part = nullptr, *h2_part = nullptr; size_t q_part_stride = 0;
    std::vector<size_t> v_off, pi_off, q_off; std::vector<int> v_chunks, pi_chunks, q_chunks;
    float* scal = nullptr;    // [0] loss_value, [1] loss_critic, [2] loss_actor (sums over the updates of one opt)
    float* samp = nullptr;    // Policy::sample rows [B][A]
    // host staging for update_on_batch
    float *u_obs = nullptr, *u_next = nullptr, *u_act = nullptr, *u_rew = nullptr; int8_t *u_term = nullptr, *u_trunc = nullptr; uint64_t u_cap = 0;
    uint64_t noise_counter = 0;
    int last_B = 0;

    ~Iql() override
    {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        free_batch();
        float* arenas[] = {pi_p, pi_g, pi_m, pi_v, v_p, v_g, v_m, v_v, scal, u_obs, u_next, u_act, u_rew};
        for (auto p : arenas) (void)hipFree(p);
        (void)hipFree(u_term); (void)hipFree(u_trunc);
        for (int i = 0; i < 4; ++i) { (void)hipFree(q_p[i]); (void)hipFree(q_t[i]); (void)hipFree(q_g[i]); (void)hipFree(q_m[i]); (void)hipFree(q_v[i]); }
    }
    void free_batch()
    {
        float** singles[] = {&x_o, &x_no, &xq, &pr_qmin1, &pr_v, &pr_u, &pr_tgt, &pr_qmin3, &pr_w, &pr_logp, &pr_vnext, &v_part, &pi_part, &q_part, &h2_part, &samp};
        for (auto p : singles) { (void)hipFree(*p); *p = nullptr; }
        for (auto* vec : {&v_act, &vo_act, &vn_act, &v_dy, &p_act, &p_dy}) { for (auto p : *vec) (void)hipFree(p); vec->clear(); }
        for (int i = 0; i < 4; ++i) for (auto* vec : {&c_act[i], &t_act[i], &c_dy[i]}) { for (auto p : *vec) (void)hipFree(p); vec->clear(); }
    }
    int32_t zalloc(float** p, size_t n)
    {
        BDR_TRY(alloc_f(p, n));
        BDR_HIP(hipMemsetAsync(*p, 0, std::max<size_t>(n, 4) * 4, stream));
        return BDR_OK;
    }
    int32_t layer_bufs(const MlpLayout& net, int Bn, std::vector<float*>& out)
    {
        for (const auto& l : net.L) { float* p = nullptr; BDR_TRY(zalloc(&p, (size_t)Bn * l.Np)); out.push_back(p); }
        return BDR_OK;
    }
    // row chunks of the grouped dW launch (k_dense_dw_small_group: 256 rows per workgroup, at most 16 chunks)
    static int chunks_for(int Bn) { return std::max(1, std::min(16, Bn / 256)); }
    static size_t plan(const MlpLayout& net, int Bn, std::vector<size_t>& off, std::vector<int>& chunks)
    {
        off.clear(); chunks.clear();
        size_t o = 0;
        for (const auto& l : net.L) { const int c = chunks_for(Bn); off.push_back(o); chunks.push_back(c); o += (size_t)c * ((size_t)l.Kp * l.Np + l.Np); }
        return o;
    }
    int32_t ensure_batch(int Bn)
    {
        if (Bn <= B) return BDR_OK;
        BDR_HIP(hipStreamSynchronize(stream));
        free_batch();
        const int Kp = vn.L[0].Kp, Kq = qn.L[0].Kp;
        BDR_TRY(zalloc(&x_o, (size_t)Bn * Kp)); BDR_TRY(zalloc(&x_no, (size_t)Bn * Kp)); BDR_TRY(zalloc(&xq, (size_t)Bn * Kq));
        for (auto* vec : {&v_act, &vo_act, &vn_act, &v_dy}) BDR_TRY(layer_bufs(vn, Bn, *vec));
        for (auto* vec : {&p_act, &p_dy}) BDR_TRY(layer_bufs(pn, Bn, *vec));
        for (int i = 0; i < NC; ++i) for (auto* vec : {&c_act[i], &t_act[i], &c_dy[i]}) BDR_TRY(layer_bufs(qn, Bn, *vec));
        float** rows[] = {&pr_qmin1, &pr_v, &pr_u, &pr_tgt, &pr_qmin3, &pr_w, &pr_logp, &pr_vnext};
        for (auto p : rows) BDR_TRY(zalloc(p, Bn));
        BDR_TRY(zalloc(&v_part, plan(vn, Bn, v_off, v_chunks)));
        BDR_TRY(zalloc(&pi_part, plan(pn, Bn, pi_off, pi_chunks)));
        q_part_stride = plan(qn, Bn, q_off, q_chunks);
        BDR_TRY(zalloc(&q_part, q_part_stride * NC));
        BDR_TRY(zalloc(&h2_part, (size_t)pad64(A)));
        BDR_TRY(zalloc(&samp, (size_t)Bn * A));
        B = Bn;
        return BDR_OK;
    }

    // forward of nz (parameters, input) pairs of one architecture, up to 4 per launch: pass j runs params[j] on x[j] into (*acts[j])[layer]
    int32_t mlp_forward(const MlpLayout& net, int n, const float* const* params, const float* const* x, std::vector<float*>* const* acts, int Bn, const char* name)
    {
        for (int j0 = 0; j0 < n; j0 += 4) {
            const int nz = std::min(4, n - j0);
            DenseSrc in[4]; float* out[4];
            for (int j = 0; j < nz; ++j) in[j] = DenseSrc{x[j0 + j], net.L[0].Kp};
            for (size_t l = 0; l < net.L.size(); ++l) {
                for (int j = 0; j < nz; ++j) out[j] = (*acts[j0 + j])[l];
                Bracket br(this, name);
                BDR_TRY(dense_forward_z(stream, net.L[l], nz, params + j0, in, out, Bn, true));
                for (int j = 0; j < nz; ++j) in[j] = DenseSrc{out[j], net.L[l].Np};
            }
        }
        return BDR_OK;
    }
    static AdamScalars opt_scalars(const bdr_adamw_config& o, double lr, uint64_t step)
    {
        return adam_scalars_for(o.opt_kind == BDR_OPT_ADAMW, lr, o.beta1, o.beta2, o.eps, o.weight_decay, step);
    }
    // backward of nz networks of one layout from the last layer's output gradient dy[z][L-1]: input gradients down to layer 1 (one
    // launch per layer for all nz), every weight gradient in one grouped launch, then the fused reduce + Adam (+ tracking into tgt)
    int32_t mlp_backward_step(const MlpLayout& net, int nz, float* const* p, float* const* g, float* const* m, float* const* v, float* const* tgt,
                              const float* x0, std::vector<float*>* const* acts, std::vector<float*>* const* dys, float* part, size_t part_stride,
                              const std::vector<size_t>& off, const AdamScalars* sc, int Bn, const char* name, size_t total, const DenseReduceSeg* extra = nullptr)
    {
        const int L = (int)net.L.size();
        for (int l = L - 1; l >= 1; --l) {
            const float* pb[4]; const float* dy[4]; float* dx[4]; const float* mask[4];
            for (int z = 0; z < nz; ++z) { pb[z] = p[z]; dy[z] = (*dys[z])[l]; dx[z] = (*dys[z])[l - 1]; mask[z] = (*acts[z])[l - 1]; }
            Bracket br(this, name);
            BDR_TRY(dense_dx_z(stream, net.L[l], nz, pb, dy, dx, mask, Bn, true));
        }
        std::vector<DenseDwJob> jobs;
        const int c = chunks_for(Bn);
        for (int z = 0; z < nz; ++z)
            for (int l = 0; l < L; ++l)
                jobs.push_back(DenseDwJob{&net.L[l], l == 0 ? DenseSrc{x0, net.L[0].Kp} : DenseSrc{(*acts[z])[l - 1], net.L[l - 1].Np}, (*dys[z])[l],
                                          part + (size_t)z * part_stride + off[l], c});
        { Bracket br(this, name); BDR_TRY(dense_dw_small_group(stream, jobs.data(), (int)jobs.size(), Bn)); }
        ReduceAdamArgs ra{};
        ra.nseg = L; ra.inst_part_stride = part_stride;
        for (int l = 0; l < L; ++l) {
            const DenseLayer& ly = net.L[l];
            const size_t nfl = (size_t)ly.Kp * ly.Np + ly.Np;
            ra.seg[l] = DenseReduceSeg{part + off[l], nfl, c, (unsigned)(ly.w / 4), (unsigned)(nfl / 4)};
        }
        if (extra) ra.seg[ra.nseg++] = *extra;
        for (int z = 0; z < nz; ++z) { ra.p[z] = p[z]; ra.g[z] = g[z]; ra.m[z] = m[z]; ra.v[z] = v[z]; ra.tgt[z] = tgt ? tgt[z] : nullptr; ra.s[z] = sc[z]; ra.vmax[z] = nullptr; }
        ra.n4 = (unsigned)(total / 4); ra.track = tgt ? 1 : 0; ra.tau = (float)cfg.critic_tau; ra.omt = (float)(1.0 - cfg.critic_tau);
        Bracket br(this, name);
        BDR_HIP(step_launch(stream, true, k_dense_reduce_adam, dim3((ra.n4 + 255) / 256, nz), dim3(256), ra));
        return BDR_OK;
    }

    // One iteration of the Iql::opt_ loop on device-resident rows (f32 obs / next_obs / act).  The reference's order is kept where a step
    // reads what the one before wrote: the value step before the critics' TD target, the soft update before the actor's advantages.
    int32_t update(int Bn, const float* obs, const float* act, const float* next_obs, const float* reward, const int8_t* term,
                   const int8_t* trunc, bool first)
    {
        BDR_TRY(ensure_batch(Bn));
        const int Lq = (int)qn.L.size(), Lv = (int)vn.L.size(), Lp = (int)pn.L.size();
        const int ldq = qn.L[Lq - 1].Np, ldv = vn.L[Lv - 1].Np;
        {
            IqlPackArgs p{obs, next_obs, act, O, A, Bn, x_o, x_no, vn.L[0].Kp, xq, qn.L[0].Kp};
            const size_t n = (size_t)Bn * (O + A);
            Bracket br(this, "pack");
            BDR_HIP(step_launch(stream, true, k_iql_pack, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), p));
        }
        // the target critics of update_value and the online critics of update_critic read the same input and parameters that no step
        // of this update has touched yet: one forward of 2 NC networks
        {
            const float* params[8]; const float* x[8]; std::vector<float*>* acts[8];
            for (int i = 0; i < NC; ++i) { params[i] = q_t[i]; x[i] = xq; acts[i] = &t_act[i]; params[NC + i] = q_p[i]; x[NC + i] = xq; acts[NC + i] = &c_act[i]; }
            BDR_TRY(mlp_forward(qn, 2 * NC, params, x, acts, Bn, "q_fwd"));
        }
        // the actor's forward needs nothing of this update but the batch
        { const float* pp[1] = {pi_p}; const float* x[1] = {x_o}; std::vector<float*>* acts[1] = {&p_act}; BDR_TRY(mlp_forward(pn, 1, pp, x, acts, Bn, "pi_fwd")); }
        // ---------------- update_value (:75-86) ----------------
        { const float* pp[1] = {v_p}; const float* x[1] = {x_o}; std::vector<float*>* acts[1] = {&v_act}; BDR_TRY(mlp_forward(vn, 1, pp, x, acts, Bn, "v_fwd")); }
        {
            IqlValueArgs p{};
            for (int i = 0; i < NC; ++i) p.qt[i] = t_act[i][Lq - 1];
            p.ldq = ldq; p.NC = NC; p.v = v_act[Lv - 1]; p.dv = v_dy[Lv - 1]; p.ldv = ldv; p.relu_out = vn.L[Lv - 1].relu;
            p.tau = (float)cfg.tau_iql; p.q_min = pr_qmin1; p.v_out = pr_v; p.u_out = pr_u; p.loss = scal; p.accumulate = first ? 0 : 1; p.B = Bn;
            Bracket br(this, "iql_value_loss");
            BDR_HIP(step_launch(stream, false, k_iql_value_loss, dim3(1), dim3(1024), p));
        }
        {
            step_v += 1;
            const AdamScalars sc = opt_scalars(cfg.opt_value, cfg.lr_value, step_v);
            std::vector<float*>* acts[1] = {&v_act}; std::vector<float*>* dys[1] = {&v_dy};
            BDR_TRY(mlp_backward_step(vn, 1, &v_p, &v_g, &v_m, &v_v, nullptr, x_o, acts, dys, v_part, 0, v_off, &sc, Bn, "v_bwd_adam", vn.total));
        }
        // ---------------- update_critic (:88-121) ----------------
        // V'(obs) (read by update_actor) and V'(next_obs) (the TD target): the same parameters, one launch per layer
        {
            const float* pp[2] = {v_p, v_p}; const float* x[2] = {x_o, x_no}; std::vector<float*>* acts[2] = {&vo_act, &vn_act};
            BDR_TRY(mlp_forward(vn, 2, pp, x, acts, Bn, "v_fwd"));
        }
        {
            IqlCriticArgs p{};
            for (int i = 0; i < NC; ++i) { p.q[i] = c_act[i][Lq - 1]; p.dq[i] = c_dy[i][Lq - 1]; }
            p.ldq = ldq; p.NC = NC; p.relu_out = qn.L[Lq - 1].relu; p.vn = vn_act[Lv - 1]; p.ldv = ldv;
            p.reward = reward; p.term = term; p.trunc = trunc; p.gamma = (float)cfg.gamma; p.tgt = pr_tgt; p.v_next = pr_vnext;
            p.loss_kind = cfg.critic_loss; p.loss = scal + 1; p.accumulate = first ? 0 : 1; p.B = Bn;
            Bracket br(this, "iql_critic_loss");
            BDR_HIP(step_launch(stream, false, k_iql_critic_loss, dim3(1), dim3(1024), p));
        }
        {
            step_q += 1;
            AdamScalars sc[4];
            std::vector<float*>* acts[4]; std::vector<float*>* dys[4];
            for (int i = 0; i < NC; ++i) { sc[i] = opt_scalars(cfg.opt_critic, cfg.lr_critic, step_q); acts[i] = &c_act[i]; dys[i] = &c_dy[i]; }
            BDR_TRY(mlp_backward_step(qn, NC, q_p, q_g, q_m, q_v, q_t, xq, acts, dys, q_part, q_part_stride, q_off, sc, Bn, "q_bwd_adam_track", qn.total));
        }
        // ---------------- update_actor (:123-155) ----------------
        {
            const float* params[4]; const float* x[4]; std::vector<float*>* acts[4];
            for (int i = 0; i < NC; ++i) { params[i] = q_t[i]; x[i] = xq; acts[i] = &t_act[i]; }
            BDR_TRY(mlp_forward(qn, NC, params, x, acts, Bn, "q_tgt_fwd"));
        }
        {
            IqlActorArgs p{};
            for (int i = 0; i < NC; ++i) p.qt[i] = t_act[i][Lq - 1];
            p.ldq = ldq; p.NC = NC; p.vo = vo_act[Lv - 1]; p.ldv = ldv;
            p.mean = p_act[Lp - 1]; p.ldm = pn.L[Lp - 1].Np; p.head2 = pi_p + h2_off; p.act = act; p.A = A;
            p.lo = (float)cfg.min_log_std; p.hi = (float)cfg.max_log_std; p.tanh_limit = cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
            p.scale = (float)cfg.action_scale; p.inv_lambda = (float)cfg.inv_lambda; p.exp_adv_max = (float)cfg.exp_adv_max; p.softmax = cfg.adv_softmax ? 1 : 0;
            p.q_min = pr_qmin3; p.w = pr_w; p.logp = pr_logp; p.gmean = p_dy[Lp - 1]; p.gh2 = h2_part;
            p.loss = scal + 2; p.accumulate = first ? 0 : 1; p.B = Bn;
            Bracket br(this, "iql_actor_loss");
            BDR_HIP(step_launch(stream, false, k_iql_actor_loss, dim3(1), dim3(1024), p));
        }
        {
            step_pi += 1;
            const AdamScalars sc = opt_scalars(cfg.opt_actor, cfg.lr_actor, step_pi);
            std::vector<float*>* acts[1] = {&p_act}; std::vector<float*>* dys[1] = {&p_dy};
            const DenseReduceSeg h2seg{h2_part, (size_t)pad64(A), 1, (unsigned)(h2_off / 4), (unsigned)(pad64(A) / 4)};
            BDR_TRY(mlp_backward_step(pn, 1, &pi_p, &pi_g, &pi_m, &pi_v, nullptr, x_o, acts, dys, pi_part, 0, pi_off, &sc, Bn, "pi_bwd_adam", pi_total, &h2seg));
        }
        n_opts += 1;
        last_B = Bn;
        return BDR_OK;
    }

    const char* kind() const override { return "iql"; }
    int32_t opt(bdr_replay* r) override
    {
        BDR_REQUIRE(r->obs_bytes == (uint64_t)O * 4 && r->act_bytes == (uint64_t)A * 4, "replay rows do not match IQL obs/act dims (f32 rows)");
        BDR_REQUIRE(r->device == device, "agent and replay buffer live on different devices");
        BDR_REQUIRE(!r->frame_stack, "IQL reads f32 observation rows, not a frame-stack store");
        const int Bn = (int)cfg.batch_size;
        BDR_TRY(ensure_batch(Bn));
        for (uint64_t u = 0; u < cfg.n_updates_per_opt; ++u) {
            { Bracket br(this, "sample"); BDR_TRY(replay_sample_on_stream(r, Bn, stream)); }
            BDR_TRY(update(Bn, (const float*)r->b_obs, (const float*)r->b_act, (const float*)r->b_next, r->b_reward, r->b_term, r->b_trunc, u == 0));
        }
        return BDR_OK;
    }
    void record_keys(std::vector<std::string>& keys) override { keys = {"loss_value", "loss_critic", "loss_actor"}; }
    int32_t gen_noise(float* dst, size_t n)
    {
        BDR_HIP(step_launch(stream, true, k_iql_randn, dim3((unsigned)((n + 255) / 256)), dim3(256), dst, n, cfg.seed, noise_counter));
        noise_counter += n;
        return BDR_OK;
    }
    int32_t noise(float* dev, size_t n) override { return gen_noise(dev, n); }   // the N(0,1) stream of Policy::sample in train mode
    int32_t record(float* out, int cap, int* n) override
    {
        float h[3];
        BDR_HIP(hipMemcpyAsync(h, scal, 12, hipMemcpyDeviceToHost, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        if (cap < 3) return fail(BDR_ERR_INVALID, "IQL record needs 3 slots");
        const float nu = (float)cfg.n_updates_per_opt;
        out[0] = h[0] / nu; out[1] = h[1] / nu; out[2] = h[2] / nu;   // loss_value, loss_critic, loss_actor (iql/base.rs:177-185)
        *n = 3;
        return BDR_OK;
    }

    // which: 0 actor, 1+i critic_i, 1+NC+i critic_tgt_i, 1+2NC value;  +100 grad, +200 exp_avg, +300 exp_avg_sq
    struct Slot { float* p; int model; size_t n; };   // model: 0 actor, 1 critic, 2 value
    Slot slot(int which)
    {
        const int role = which / 100, id = which % 100;
        if (role > 3 || which < 0) return Slot{nullptr, 0, 0};
        if (id == 0) { float* r[4] = {pi_p, pi_g, pi_m, pi_v}; return Slot{r[role], 0, pi_total}; }
        if (id >= 1 && id <= NC) { const int i = id - 1; float* r[4] = {q_p[i], q_g[i], q_m[i], q_v[i]}; return Slot{r[role], 1, qn.total}; }
        if (id >= 1 + NC && id <= 2 * NC && role == 0) return Slot{q_t[id - 1 - NC], 1, qn.total};
        if (id == 1 + 2 * NC) { float* r[4] = {v_p, v_g, v_m, v_v}; return Slot{r[role], 2, vn.total}; }
        return Slot{nullptr, 0, 0};
    }
    uint64_t param_count(int which) override
    {
        Slot s = slot(which);
        if (!s.p) return 0;
        return s.model == 0 ? pn.ref_total + (uint64_t)A : s.model == 1 ? qn.ref_total : vn.ref_total;
    }
    int32_t get_params(int which, float* out, uint64_t n) override
    {
        Slot s = slot(which);
        BDR_REQUIRE(s.p, "unknown IQL model %d", which);
        BDR_REQUIRE(n == param_count(which), "parameter count mismatch (%llu vs %llu)", (unsigned long long)n, (unsigned long long)param_count(which));
        std::vector<float> in(s.n);
        BDR_HIP(hipMemcpyAsync(in.data(), s.p, s.n * 4, hipMemcpyDeviceToHost, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        if (s.model == 0) { mlp_to_reference(pn, 0, in.data(), out); for (int j = 0; j < A; ++j) out[pn.ref_total + j] = in[h2_off + j]; }
        else mlp_to_reference(s.model == 1 ? qn : vn, 0, in.data(), out);
        return BDR_OK;
    }
    int32_t set_params(int which, const float* inp, uint64_t n) override
    {
        Slot s = slot(which);
        BDR_REQUIRE(s.p, "unknown IQL model %d", which);
        BDR_REQUIRE(n == param_count(which), "parameter count mismatch");
        std::vector<float> in(s.n, 0.f);
        if (s.model == 0) { mlp_to_internal(pn, 0, inp, in.data()); for (int j = 0; j < A; ++j) in[h2_off + j] = inp[pn.ref_total + j]; }
        else mlp_to_internal(s.model == 1 ? qn : vn, 0, inp, in.data());
        BDR_HIP(hipMemcpyAsync(s.p, in.data(), s.n * 4, hipMemcpyHostToDevice, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        return BDR_OK;
    }
    // SyncModel ships the actor (model 0)
    float* arena(int which, size_t* n) override { Slot s = slot(which); if (n) *n = s.n; return s.p; }

    static void mlp_meta(const MlpLayout& net, const std::string& prefix, std::vector<NamedTensor>& mt)
    {
        for (size_t i = 0; i < net.L.size(); ++i) {
            mt.push_back({prefix + "mlp.ln" + std::to_string(i) + ".weight", {(uint64_t)net.L[i].out, (uint64_t)net.L[i].in}});
            mt.push_back({prefix + "mlp.ln" + std::to_string(i) + ".bias", {(uint64_t)net.L[i].out}});
        }
    }
    std::vector<NamedTensor> actor_meta() const
    {
        std::vector<NamedTensor> mt;
        mlp_meta(pn, "actor.", mt);
        mt.push_back({"actor.head2", {1, (uint64_t)A}});
        return mt;
    }
    std::vector<NamedTensor> critic_meta() const   // one VarMap holds every critic: critic{i}.mlp.ln{k}.* (util/critic.rs:155-170)
    {
        std::vector<NamedTensor> mt;
        for (int i = 0; i < NC; ++i) mlp_meta(qn, "critic" + std::to_string(i) + ".", mt);
        return mt;
    }
    std::vector<NamedTensor> value_meta() const { std::vector<NamedTensor> mt; mlp_meta(vn, "value.", mt); return mt; }
    // candle's VarMap::save writes safetensors whatever the extension: "<stem>.pt" (default, the reference's files) or "<stem>.safetensors"
    std::string save_path(const char* dir, const char* stem) const { return std::string(dir) + "/" + stem + (ckpt_format == BDR_CKPT_SAFETENSORS ? ".safetensors" : ".pt"); }
    std::string load_path(const char* dir, const char* stem) const
    {
        const std::string first = save_path(dir, stem);
        const std::string second = std::string(dir) + "/" + stem + (ckpt_format == BDR_CKPT_SAFETENSORS ? ".pt" : ".safetensors");
        FILE* f = fopen(first.c_str(), "rb");
        if (f) { fclose(f); return first; }
        f = fopen(second.c_str(), "rb");
        if (f) { fclose(f); return second; }
        return first;
    }
    int32_t save(const char* dir) override   // iql/base.rs:292-302: actor, critic, critic.tgt, value
    {
        std::vector<float> v(param_count(0));
        BDR_TRY(get_params(0, v.data(), v.size()));
        BDR_TRY(save_safetensors_named(save_path(dir, "actor"), actor_meta(), v.data(), v.size()));
        const size_t nq = qn.ref_total;
        v.assign((size_t)NC * nq, 0.f);
        for (int i = 0; i < NC; ++i) BDR_TRY(get_params(1 + i, v.data() + (size_t)i * nq, nq));
        BDR_TRY(save_safetensors_named(save_path(dir, "critic"), critic_meta(), v.data(), v.size()));
        BDR_TRY(save_safetensors_named(save_path(dir, "critic.tgt"), critic_meta(), v.data(), v.size()));   // the ONLINE critics (util/critic.rs:272-285)
        v.resize(vn.ref_total);
        BDR_TRY(get_params(1 + 2 * NC, v.data(), v.size()));
        return save_safetensors_named(save_path(dir, "value"), value_meta(), v.data(), v.size());
    }
    int32_t load(const char* dir) override   // iql/base.rs:304-309
    {
        std::vector<float> v(param_count(0));
        BDR_TRY(load_safetensors_named(load_path(dir, "actor"), actor_meta(), v.data(), v.size()));
        BDR_TRY(set_params(0, v.data(), v.size()));
        const size_t nq = qn.ref_total;
        v.assign((size_t)NC * nq, 0.f);
        // MultiCritic::load (util/critic.rs:287-298): both files into the ONLINE critics' VarMap - the second load wins - and the
        // targets stay as they are
        BDR_TRY(load_safetensors_named(load_path(dir, "critic"), critic_meta(), v.data(), v.size()));
        BDR_TRY(load_safetensors_named(load_path(dir, "critic.tgt"), critic_meta(), v.data(), v.size()));
        for (int i = 0; i < NC; ++i) BDR_TRY(set_params(1 + i, v.data() + (size_t)i * nq, nq));
        v.resize(vn.ref_total);
        BDR_TRY(load_safetensors_named(load_path(dir, "value"), value_meta(), v.data(), v.size()));
        return set_params(1 + 2 * NC, v.data(), v.size());
    }
};

namespace {
int32_t check_mlp(const bdr_mlp_config& m, const char* what, bool actor)
{
    BDR_REQUIRE(m.n_units >= (actor ? 1 : 0) && m.n_units <= BDR_MAX_UNITS, "%s: bad layer count", what);
    for (int i = 0; i < m.n_units; ++i) BDR_REQUIRE(m.units[i] >= 1 && m.units[i] <= 4096, "%s: bad layer width", what);
    BDR_REQUIRE(m.activation_out == BDR_ACTIVATION_NONE || m.activation_out == BDR_ACTIVATION_RELU,
                "%s: activation_out must be None or ReLU (Tanh / Sigmoid are not supported)", what);
    return BDR_OK;
}
int32_t check_opt(const bdr_adamw_config& o, const char* what)
{
    BDR_REQUIRE(o.opt_kind == BDR_OPT_ADAM || o.opt_kind == BDR_OPT_ADAMW, "%s: unknown optimizer", what);
    BDR_REQUIRE(!(o.opt_kind == BDR_OPT_ADAMW && o.amsgrad), "%s: candle's AdamW has no amsgrad", what);
    return BDR_OK;
}
}  // namespace

extern "C" {

void bdr_iql_config_default(bdr_iql_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    // iql/config.rs:109-125
    c->gamma = 0.99; c->tau_iql = 0.7; c->inv_lambda = 10.0; c->n_updates_per_opt = 1; c->batch_size = 1; c->adv_softmax = 0;
    c->critic_loss = BDR_LOSS_MSE; c->exp_adv_max = 100.0; c->device = -1; c->train = 0;
    // MultiCriticConfig (util/critic.rs:35-43), GaussianActorConfig (util/actor.rs:44-55), ValueConfig (iql/value.rs)
    c->n_critics = 2; c->critic_tau = 0.005;
    c->lr_value = c->lr_actor = c->lr_critic = 3e-4;
    c->min_log_std = -20.0; c->max_log_std = 2.0;
    c->action_limit = BDR_ACTION_LIMIT_CLAMP; c->action_min = -1.0; c->action_max = 1.0; c->action_scale = 1.0;
    for (bdr_adamw_config* o : {&c->opt_value, &c->opt_actor, &c->opt_critic}) { o->opt_kind = BDR_OPT_ADAM; o->beta1 = 0.9; o->beta2 = 0.999; o->weight_decay = 0.01; o->eps = 1e-8; }
    for (bdr_mlp_config* m : {&c->value, &c->actor, &c->critic}) m->activation_out = BDR_ACTIVATION_NONE;
}

int32_t bdr_iql_create(const bdr_iql_config* cfg, bdr_agent** out)
{
    BDR_REQUIRE(cfg && out, "null argument");
    BDR_REQUIRE(cfg->device >= 0, "No device is given for IQL agent");
    BDR_REQUIRE(cfg->obs_dim >= 1 && cfg->obs_dim <= 4096 && cfg->act_dim >= 1 && cfg->act_dim <= 256, "bad obs/act dims");
    BDR_TRY(check_mlp(cfg->value, "value", false));
    BDR_TRY(check_mlp(cfg->actor, "actor (Mlp3)", true));
    BDR_TRY(check_mlp(cfg->critic, "critic", false));
    BDR_REQUIRE(cfg->n_critics >= 1 && cfg->n_critics <= 4, "n_critics must be in [1,4]");
    BDR_REQUIRE(cfg->batch_size >= 1 && cfg->batch_size <= 65536 && cfg->n_updates_per_opt >= 1, "bad batch / update counts");
    BDR_REQUIRE(cfg->action_limit == BDR_ACTION_LIMIT_CLAMP || cfg->action_limit == BDR_ACTION_LIMIT_TANH, "unknown action limit");
    BDR_REQUIRE(cfg->critic_loss == BDR_LOSS_MSE || cfg->critic_loss == BDR_LOSS_SMOOTH_L1, "unknown critic loss");
    BDR_TRY(check_opt(cfg->opt_value, "value")); BDR_TRY(check_opt(cfg->opt_actor, "actor")); BDR_TRY(check_opt(cfg->opt_critic, "critic"));
    BDR_TRY(ensure_device(cfg->device));
    Iql* a = new Iql();
    a->cfg = *cfg; a->device = cfg->device; a->train = cfg->train != 0;
    a->O = cfg->obs_dim; a->A = cfg->act_dim; a->NC = cfg->n_critics;
    a->vn = make_mlp(a->O, cfg->value.units, cfg->value.n_units, 1, cfg->value.activation_out == BDR_ACTIVATION_RELU);
    a->pn = make_mlp(a->O, cfg->actor.units, cfg->actor.n_units, a->A, false);   // Mlp3: no output activation
    a->qn = make_mlp(a->O + a->A, cfg->critic.units, cfg->critic.n_units, 1, cfg->critic.activation_out == BDR_ACTIVATION_RELU);
    a->h2_off = a->pn.total; a->pi_total = a->pn.total + (size_t)pad64(a->A);
    const int32_t st = [&]() -> int32_t {
        BDR_HIP(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
        BDR_TRY(a->err_init());
        for (auto p : {&a->pi_p, &a->pi_g, &a->pi_m, &a->pi_v}) BDR_TRY(a->zalloc(p, a->pi_total));
        for (auto p : {&a->v_p, &a->v_g, &a->v_m, &a->v_v}) BDR_TRY(a->zalloc(p, a->vn.total));
        for (int i = 0; i < a->NC; ++i)
            for (auto p : {&a->q_p[i], &a->q_t[i], &a->q_g[i], &a->q_m[i], &a->q_v[i]}) BDR_TRY(a->zalloc(p, a->qn.total));
        BDR_TRY(a->zalloc(&a->scal, 4));
        // initial parameters: the library's initialiser, head2 = 0 (mlp3.rs: Init::Const(0.)); targets are copies of the critics
        std::vector<float> ref(a->param_count(0), 0.f);
        mlp_init_reference(a->pn, cfg->seed * 7 + 1, ref.data());
        BDR_TRY(a->set_params(0, ref.data(), ref.size()));
        ref.assign(a->qn.ref_total, 0.f);
        for (int i = 0; i < a->NC; ++i) {
            mlp_init_reference(a->qn, cfg->seed * 7 + 2 + i, ref.data());
            BDR_TRY(a->set_params(1 + i, ref.data(), ref.size()));
            BDR_TRY(a->set_params(1 + a->NC + i, ref.data(), ref.size()));
        }
        ref.assign(a->vn.ref_total, 0.f);
        mlp_init_reference(a->vn, cfg->seed * 7 + 6, ref.data());
        BDR_TRY(a->set_params(1 + 2 * a->NC, ref.data(), ref.size()));
        return a->ensure_batch((int)cfg->batch_size);
    }();
    if (st != BDR_OK) { delete a; return st; }
    *out = a;
    return BDR_OK;
}

int32_t bdr_iql_update_on_batch(bdr_agent* base, uint64_t n, const float* obs, const float* act, const float* next_obs,
                                const float* reward, const int8_t* term, const int8_t* trunc, float* rec3)
{
    BDR_REQUIRE(base && obs && act && next_obs && reward && term && trunc, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "iql"), "not an IQL agent");
    BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
    Iql* a = static_cast<Iql*>(base);
    BDR_HIP(hipSetDevice(a->device));
    BDR_TRY(a->ensure_batch((int)n));
    if (n > a->u_cap) {
        BDR_HIP(hipStreamSynchronize(a->stream));
        (void)hipFree(a->u_obs); (void)hipFree(a->u_next); (void)hipFree(a->u_act); (void)hipFree(a->u_rew); (void)hipFree(a->u_term); (void)hipFree(a->u_trunc);
        a->u_obs = a->u_next = a->u_act = a->u_rew = nullptr; a->u_term = a->u_trunc = nullptr; a->u_cap = 0;
        BDR_HIP(hipMalloc((void**)&a->u_obs, n * a->O * 4)); BDR_HIP(hipMalloc((void**)&a->u_next, n * a->O * 4));
        BDR_HIP(hipMalloc((void**)&a->u_act, n * a->A * 4)); BDR_HIP(hipMalloc((void**)&a->u_rew, n * 4));
        BDR_HIP(hipMalloc((void**)&a->u_term, round_up(n, 16))); BDR_HIP(hipMalloc((void**)&a->u_trunc, round_up(n, 16)));
        a->u_cap = n;
    }
    hipStream_t s = a->stream;
    BDR_HIP(hipMemcpyAsync(a->u_obs, obs, n * a->O * 4, hipMemcpyHostToDevice, s));
    BDR_HIP(hipMemcpyAsync(a->u_next, next_obs, n * a->O * 4, hipMemcpyHostToDevice, s));
    BDR_HIP(hipMemcpyAsync(a->u_act, act, n * a->A * 4, hipMemcpyHostToDevice, s));
    BDR_HIP(hipMemcpyAsync(a->u_rew, reward, n * 4, hipMemcpyHostToDevice, s));
    BDR_HIP(hipMemcpyAsync(a->u_term, term, n, hipMemcpyHostToDevice, s));
    BDR_HIP(hipMemcpyAsync(a->u_trunc, trunc, n, hipMemcpyHostToDevice, s));
    BDR_TRY(a->update((int)n, a->u_obs, a->u_act, a->u_next, a->u_rew, a->u_term, a->u_trunc, true));
    prof_collect(a);
    if (rec3) {
        float h[3];
        BDR_HIP(hipMemcpyAsync(h, a->scal, 12, hipMemcpyDeviceToHost, s));
        BDR_HIP(hipStreamSynchronize(s));
        rec3[0] = h[0]; rec3[1] = h[1]; rec3[2] = h[2];
    } else {
        BDR_HIP(hipStreamSynchronize(s));
    }
    return a->err_check();
}

// Parity probes of the LAST update (see include/border_amd.h)
int32_t bdr_iql_probe(bdr_agent* base, int32_t what, float* out, uint64_t n)
{
    BDR_REQUIRE(base && out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "iql"), "not an IQL agent");
    Iql* a = static_cast<Iql*>(base);
    BDR_HIP(hipSetDevice(a->device));
    const int Bn = a->last_B, NC = a->NC;
    BDR_REQUIRE(Bn > 0, "no update has run yet");
    BDR_HIP(hipStreamSynchronize(a->stream));
    auto column0 = [&](const float* m, int ld, float* dst) -> int32_t {   // [Bn][ld] -> [Bn]
        std::vector<float> h((size_t)Bn * ld);
        BDR_HIP(hipMemcpy(h.data(), m, h.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < Bn; ++b) dst[b] = h[(size_t)b * ld];
        return BDR_OK;
    };
    const float* rows[10] = {a->pr_qmin1, a->pr_v, a->pr_u, a->pr_tgt, nullptr, a->pr_qmin3, a->pr_w, a->pr_logp, a->pr_vnext, nullptr};
    if (what < 0 || what > 9) return fail(BDR_ERR_INVALID, "unknown IQL probe %d", what);
    if (what == 4) {   // Q_i(obs, act) of update_critic
        BDR_REQUIRE(n == (uint64_t)NC * Bn, "q_pred holds n_critics x batch values");
        const int Lq = (int)a->qn.L.size();
        for (int i = 0; i < NC; ++i) BDR_TRY(column0(a->c_act[i][Lq - 1], a->qn.L[Lq - 1].Np, out + (size_t)i * Bn));
        return BDR_OK;
    }
    BDR_REQUIRE(n == (uint64_t)Bn, "this probe holds batch values");
    if (what == 9) { const int Lv = (int)a->vn.L.size(); return column0(a->vo_act[Lv - 1], a->vn.L[Lv - 1].Np, out); }
    BDR_HIP(hipMemcpy(out, rows[what], (size_t)Bn * 4, hipMemcpyDeviceToHost));
    return BDR_OK;
}

// Policy::sample (util/actor.rs:226-241); out: [n][act_dim]
int32_t bdr_iql_sample(bdr_agent* base, uint64_t n, const float* obs, float* act_out)
{
    BDR_REQUIRE(base && obs && act_out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "iql"), "not an IQL agent");
    BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
    Iql* a = static_cast<Iql*>(base);
    BDR_HIP(hipSetDevice(a->device));
    BDR_TRY(a->ensure_batch((int)n));
    const float* d = nullptr;
    int32_t st = BDR_OK;
    if (!a->obs_rows_on_device && n * a->O * 4 <= bdr_agent::HOST_ROWS_PINNED_MAX) {   // host rows: read in place from pinned memory by the packing kernel
        const uint8_t* pd = nullptr;
        BDR_TRY(a->host_rows_pinned(obs, n * a->O * 4, &pd));
        d = reinterpret_cast<const float*>(pd);
    } else {
        float* stage = nullptr;
        BDR_TRY(a->act_buffer(n * a->O * 4, (void**)&stage));
        st = a->stage_obs(stage, obs, (size_t)a->O * 4, n, a->stream);
        d = stage;
    }
    const int Lp = (int)a->pn.L.size();
    if (st == BDR_OK) st = pack_rows(a->stream, d, a->O, a->O, a->x_o, a->pn.L[0].Kp, 0, (int)n);
    if (st == BDR_OK) {
        const float* pp[1] = {a->pi_p}; const float* x[1] = {a->x_o}; std::vector<float*>* acts[1] = {&a->p_act};
        st = a->mlp_forward(a->pn, 1, pp, x, acts, (int)n, "pi_fwd");
    }
    if (st == BDR_OK) {
        IqlSampleArgs p{};
        p.mean = a->p_act[Lp - 1]; p.ldm = a->pn.L[Lp - 1].Np; p.head2 = a->pi_p + a->h2_off; p.A = a->A; p.n = (int)n;
        p.lo = (float)a->cfg.min_log_std; p.hi = (float)a->cfg.max_log_std; p.tanh_limit = a->cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
        p.amin = (float)a->cfg.action_min; p.amax = (float)a->cfg.action_max; p.scale = (float)a->cfg.action_scale;
        p.train = a->train ? 1 : 0; p.seed = a->cfg.seed; p.counter = a->noise_counter; p.out = a->samp;
        if (a->train) a->noise_counter += n * a->A;
        const int tot = (int)n * a->A;
        hipLaunchKernelGGL(k_iql_sample, dim3((tot + 255) / 256), dim3(256), 0, a->stream, p);
        if (hipGetLastError() != hipSuccess) st = fail(BDR_ERR_HIP, "sample launch failed");
    }
    if (st == BDR_OK) st = a->rows_to_host(a->samp, act_out, n * a->A);
    a->slot_cursor = 0;
    return st;
}

int32_t bdr_iql_sample_device(bdr_agent* base, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out)
{
    BDR_REQUIRE(base && obs_dev && act_out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "iql"), "not an IQL agent");
    BDR_REQUIRE(row_stride >= (uint64_t)static_cast<Iql*>(base)->O * 4 && row_stride % 4 == 0, "row_stride must be >= the row size and a multiple of 4");
    BDR_HIP(hipSetDevice(base->device));
    BDR_TRY(base->check_device_rows(obs_dev, row_stride));
    bdr_agent::DeviceRowsScope rows(base, row_stride);
    return bdr_iql_sample(base, n, static_cast<const float*>(obs_dev), act_out);
}

}  // extern "C"
