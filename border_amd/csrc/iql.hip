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

using namespace bdr;

namespace {

// obs / next_obs / act rows -> the zero-padded inputs of the value + actor ([B][Kp], obs and next_obs) and of the critics ([B][Kq], obs | act)
struct IqlPackArgs { const float* obs; const float* next; const float* act; int O, A, B; float* x_o; float* x_no; int ldp; float* xq; int ldq; };
// (the bodies of the four kernels below are functions over their argument struct: the kernel argument, or a member's entry of a device
// array read in place - iql_group.hpp, where blockIdx.y is the member; `red` is the kernel's own 32 floats of LDS)
template <class Args>
__device__ __forceinline__ void iql_pack_body(const Args& p)
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
__global__ __launch_bounds__(256) void k_iql_pack(IqlPackArgs p) { iql_pack_body(p); }

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
template <class Args>
__device__ __forceinline__ void iql_value_loss_body(const Args& p, float* red)
{
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
__global__ __launch_bounds__(1024) void k_iql_value_loss(IqlValueArgs p)
{
    __shared__ float red[32];
    iql_value_loss_body(p, red);
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
template <class Args>
__device__ __forceinline__ void iql_critic_loss_body(const Args& p, float* red)
{
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
            candle::critic_loss_elem(p.loss_kind, d, l, g);
            float gq = g * scale;
            if (p.relu_out && !(q > 0.f)) gq = 0.f;
            p.dq[i][(size_t)b * p.ldq] = gq;
            return l;
        }, red);
        total = candle::acc(total, si, scale);
    }
    if (threadIdx.x == 0) p.loss[0] = total;
}
__global__ __launch_bounds__(1024) void k_iql_critic_loss(IqlCriticArgs p)
{
    __shared__ float red[32];
    iql_critic_loss_body(p, red);
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
template <class Args>
__device__ __forceinline__ float iql_x(const Args& p, float a)
{
#pragma clang fp contract(off)
    if (!p.tanh_limit) return a;
    const float t = fminf(fmaxf(a / p.scale, -0.999999f), 0.999999f);   // util.rs:268-271 atanh
    const float r = (1.0f + t) / (1.0f - t);
    return 0.5f * logf(r);
}
template <class Args>
__device__ __forceinline__ void iql_actor_loss_body(const Args& p, float* red)
{
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
__global__ __launch_bounds__(1024) void k_iql_actor_loss(IqlActorArgs p)
{
    __shared__ float red[32];
    iql_actor_loss_body(p, red);
}

}  // namespace


// ================================================================================================
// The actor, the critics and their steps, Policy::sample, the parameter views and the checkpoints' actor and critic files are
// CandleAgent's (candle_actor.hpp); IQL adds the value network (model 1 + 2NC, value.pt) and its update schedule.
struct Iql : CandleAgent<Iql, bdr_iql_config> {
    static constexpr const char* NAME = "IQL";
    static constexpr int N_RECORD = 3;   // scal: [0] loss_value, [1] loss_critic, [2] loss_actor (sums over the updates of one opt)
    MlpLayout vn;                        // value
    float *v_p = nullptr, *v_g = nullptr, *v_m = nullptr, *v_v = nullptr;
    uint64_t step_v = 0;
    // batch buffers
    std::vector<float*> v_act, vo_act, vn_act, v_dy;          // V(obs) (step 1), V'(obs), V'(next_obs); value gradients
    float *pr_qmin1 = nullptr, *pr_v = nullptr, *pr_u = nullptr, *pr_qmin3 = nullptr, *pr_vnext = nullptr;
    float* v_part = nullptr; std::vector<size_t> v_off;

    int32_t init_own()   // the value network: iql/value.rs, initial parameters at seed * 7 + 6
    {
        vn = make_mlp(O, cfg.value.units, cfg.value.n_units, 1, cfg.value.activation_out == BDR_ACTIVATION_RELU);
        for (auto p : {&v_p, &v_g, &v_m, &v_v}) BDR_TRY(alloc(p, vn.total, AGENT));
        std::vector<float> ref(vn.ref_total, 0.f);
        mlp_init_reference(vn, cfg.seed * 7 + 6, ref.data());
        return set_params(1 + 2 * NC, ref.data(), ref.size());
    }
    bool own_view(int k, int role, ParamView* pv)
    {
        float* r[4] = {v_p, v_g, v_m, v_v};
        if (k == 0) *pv = mlp_view(vn, r[role]);
        return k == 0;
    }
    void own_files(std::vector<CheckpointFile>& files)   // iql/base.rs:292-309: actor, critic, critic.tgt, value
    {
        std::vector<NamedTensor> mt;
        mlp_meta(vn, "value.", mt);
        files.push_back({"value", mt, {1 + 2 * NC}, {1 + 2 * NC}});
    }
    void own_arenas(std::vector<StateArena>& out) { for (float* a : {v_p, v_g, v_m, v_v}) out.push_back({a, vn.total}); }
    void own_steps(const Iql& s) { step_v = s.step_v; }
    double* own_hyper(int32_t id)
    {
        if (id >= BDR_HYPER_LR_VALUE && id <= BDR_HYPER_VALUE_WEIGHT_DECAY) return opt_field(cfg.opt_value, cfg.lr_value, id - BDR_HYPER_LR_VALUE);
        return id == BDR_HYPER_TAU_IQL ? &cfg.tau_iql : id == BDR_HYPER_INV_LAMBDA ? &cfg.inv_lambda : id == BDR_HYPER_EXP_ADV_MAX ? &cfg.exp_adv_max : nullptr;
    }
    int32_t alloc_batch(int Bn)
    {
        for (auto* vec : {&v_act, &vo_act, &vn_act, &v_dy}) BDR_TRY(layer_bufs(vn, Bn, *vec));
        for (auto p : {&pr_qmin1, &pr_v, &pr_u, &pr_qmin3, &pr_vnext}) BDR_TRY(alloc(p, Bn, BATCH));
        return alloc(&v_part, plan(vn, Bn, v_off), BATCH);
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
        BDR_TRY(actor_forward(x_o, p_act, Bn));
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
        BDR_TRY(critic_step(Bn));
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
        BDR_TRY(actor_step(Bn));
        n_opts += 1;
        last_B = Bn;
        return BDR_OK;
    }

    const char* kind() const override { return "iql"; }
    void record_keys(std::vector<std::string>& keys) override { keys = {"loss_value", "loss_critic", "loss_actor"}; }
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
};

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
    return Iql::create(*cfg, out, &cfg->value, &cfg->opt_value, nullptr);
}

int32_t bdr_iql_update_on_batch(bdr_agent* base, uint64_t n, const float* obs, const float* act, const float* next_obs,
                                const float* reward, const int8_t* term, const int8_t* trunc, float* rec3)
{
    BDR_REQUIRE(base && obs && act && next_obs && reward && term && trunc, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "iql"), "not an IQL agent");
    BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
    Iql* a = static_cast<Iql*>(base);
    BDR_TRY(a->stage_batch(n, obs, act, next_obs, reward, term, trunc));
    BDR_TRY(a->update((int)n, a->u_obs, a->u_act, a->u_next, a->u_rew, a->u_term, a->u_trunc, true));
    return a->batch_done(rec3);
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
    return static_cast<Iql*>(base)->sample(n, obs, act_out);
}

int32_t bdr_iql_sample_device(bdr_agent* base, uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out)
{
    BDR_REQUIRE(base && obs_dev && act_out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "iql"), "not an IQL agent");
    return static_cast<Iql*>(base)->sample_device(n, obs_dev, row_stride, act_out);
}

}  // extern "C"

// ================================================================================================
// the launch grouping of IQL agents (bdr_iql_group_*): it needs Iql and the kernel bodies above
#include "iql_group.hpp"
