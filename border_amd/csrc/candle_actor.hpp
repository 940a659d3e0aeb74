// The candle-family agents (IQL: iql.hip, AWAC: awac.hip, SAC: candle_sac.hip) share a GaussianActor (util/actor.rs) over Mlp3
// (mlp/mlp3.rs; SAC also over Mlp2, mlp/mlp2.rs: the two heads are one last layer of width 2 A, mean columns then s columns) and a
// MultiCritic of Mlp on cat(obs, act) with soft-updated targets (util/critic.rs), trained on the FP32-MFMA kernels of dense.hpp.
// This header holds what they share.  Device: the counter-based N(0,1) noise stream of Policy::sample, the fixed-order batch sums
// (BC's loss, bc.hip, uses their butterfly and acc too) and the sample kernel.  Host: CandleAgent, the actor + critics + targets
// core each of the two derives from, itself on DenseAgent (dense_agent.hpp: buffer lifetimes, the Mlp forward and backward step,
// the observation rows of an acting call, the reference layout); an agent adds its update schedule, its loss kernels, its records
// and probes, and any model of its own.  Every batch-wide sum is formed in one order (rows in blocks of 32, a 32-lane butterfly per
// block, the block partials added in block order), so an update gives the same bits run to run.
#pragma once
#include "dense_agent.hpp"

namespace bdr {
namespace candle {

// (the counter-based N(0,1) of the agent's noise stream, randn_at, lives in dense_act.hpp beside the element code of Policy::sample)

// ---- fixed-order batch sums (one 1024-thread workgroup) ----------------------------------------------------------------------
__device__ __forceinline__ float butterfly32(float v)
{
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// sum over b < B of value(b): rows in blocks of 32, each block's butterfly, the partials added in block order
template <class F>
__device__ __forceinline__ float row_sum(int B, F&& value, float* red32)
{
    float total = 0.f;
    for (int base = 0; base < B; base += 1024) {
        const int b = base + (int)threadIdx.x;
        const float part = butterfly32(b < B ? value(b) : 0.f);
        if ((threadIdx.x & 31) == 0) red32[threadIdx.x >> 5] = part;
        __syncthreads();
        const int nb = min(32, (B - base + 31) / 32);
        for (int k = 0; k < nb; ++k) total += red32[k];
        __syncthreads();
    }
    return total;
}
template <class F>
__device__ __forceinline__ float row_max(int B, F&& value, float* red32)
{
    float m = -INFINITY;
    for (int base = 0; base < B; base += 1024) {
        const int b = base + (int)threadIdx.x;
        float v = b < B ? value(b) : -INFINITY;
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
        if ((threadIdx.x & 31) == 0) red32[threadIdx.x >> 5] = v;
        __syncthreads();
        const int nb = min(32, (B - base + 31) / 32);
        for (int k = 0; k < nb; ++k) m = fmaxf(m, red32[k]);
        __syncthreads();
    }
    return m;
}
// The critic-loss element of every candle agent's update_critic (candle_nn::loss::mse, util.rs:144-152 smooth_l1_loss with beta 1):
// d = pred - tgt -> the loss element l and dl/dpred g, before the mean's scale.  One definition for IQL, AWAC, SAC and DQN.
__device__ __forceinline__ void critic_loss_elem(int loss_kind, float d, float& l, float& g)
{
#pragma clang fp contract(off)
    if (loss_kind == 1) { const float z = fabsf(d); const float hz = 0.5f * z; l = z < 1.f ? hz * z : z - 0.5f; g = z < 1.f ? d : (d > 0.f ? 1.f : -1.f); }
    else { l = d * d; g = 2.f * d; }
}
__device__ __forceinline__ float acc(float base, float s, float scale)   // base + s * scale, rounded step by step
{
#pragma clang fp contract(off)
    const float t = s * scale;
    return base + t;
}

}  // namespace candle
}  // namespace bdr

namespace {
using namespace bdr;

__global__ void k_candle_randn(float* __restrict__ out, size_t n, uint64_t seed, uint64_t counter)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = candle::randn_at(seed, counter, i);
}

// Policy::sample (util/actor.rs:226-241): train: mean + std z, eval: mean; then clamp or scale * tanh.  z = the host draws z[t] when
// given, else the device stream at counter + t (t = b * A + j).  out [n][A]; xq (optional): the action columns O.. of a critic input.
struct CandleSampleArgs {
    const float* mean; int ldm; int A, n;
    SampleElem e;   // the element code and its operands (dense_act.hpp: shared with k_dense_act)
    float* out; float* xq; int ldq; int O;
};
// (the body over its argument struct: the kernel argument, or a member's entry of a device array read in place - awac_group.hpp, where
// blockIdx.y is the member and `e` is built in registers from the entry's static half and the member's step slot)
template <class Args>
__device__ __forceinline__ void candle_sample_body(const Args& p, const SampleElem& e)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.n * p.A) return;
    const int b = t / p.A, j = t % p.A;
    const float* row = p.mean + (size_t)b * p.ldm;
    const float a = candle_sample_elem(e, row[j], j, (size_t)t, e.mlp2 ? row[p.A + j] : 0.f);
    p.out[t] = a;
    if (p.xq) p.xq[(size_t)b * p.ldq + p.O + j] = a;
}
__global__ __launch_bounds__(256) void k_candle_sample(CandleSampleArgs p) { candle_sample_body(p, p.e); }

int32_t check_mlp(const bdr_mlp_config& m, const char* what, bool actor)
{
    BDR_REQUIRE(m.n_units >= (actor ? 1 : 0) && m.n_units <= BDR_MAX_UNITS, "%s: bad layer count", what);
    for (int i = 0; i < m.n_units; ++i) BDR_REQUIRE(m.units[i] >= 1 && m.units[i] <= 4096, "%s: bad layer width", what);
    BDR_REQUIRE(m.activation_out == BDR_ACTIVATION_NONE || m.activation_out == BDR_ACTIVATION_RELU,
                "%s: activation_out must be None or ReLU (Tanh / Sigmoid are not supported)", what);
    return BDR_OK;
}

// ================================================================================================
// The host core.  Self is the agent (CRTP): it supplies NAME (in messages), N_RECORD (its record values), kind(), record(),
// record_keys(), update(Bn, obs, act, next_obs, reward, term, trunc, first) and alloc_batch(Bn), and may replace the hooks
// init_own, alloc_staging, own_view and own_files below.  Cfg is its bdr_*_config; the fields named here are common to all of them.
template <class Self, class Cfg>
struct CandleAgent : DenseAgent {
    Cfg cfg;
    int NC = 2;
    int actor_kind = BDR_ACTOR_MLP3;   // BDR_ACTOR_MLP2: pn's last layer is [mean | s] (2 A columns) and there is no head2
    MlpLayout pn, qn;                  // actor mean (head2 follows pn in the actor arena), critic
    size_t h2_off = 0, pi_total = 0;   // head2 at h2_off (= pn.total) in the actor arena; pi_total = pn.total + pad64(A) (Mlp2: pn.total)
    bool mlp2() const { return actor_kind == BDR_ACTOR_MLP2; }
    // arenas: parameters, gradients, exp_avg, exp_avg_sq (+ the critics' targets)
    float *pi_p = nullptr, *pi_g = nullptr, *pi_m = nullptr, *pi_v = nullptr;
    float* q_p[4] = {nullptr}; float* q_t[4] = {nullptr}; float* q_g[4] = {nullptr}; float* q_m[4] = {nullptr}; float* q_v[4] = {nullptr};
    uint64_t step_pi = 0, step_q = 0;
    uint64_t noise_counter = 0;
    // batch buffers (ensure_batch)
    int B = 0; uint64_t batch_gen = 0;   // batch_gen: bumped whenever the batch buffers are re-allocated (iql_group.hpp and awac_group.hpp key their static arguments on it)
    float *x_o = nullptr, *x_no = nullptr, *xq = nullptr;    // actor inputs [B][Kp] (obs, next_obs), critic input [B][Kq] (obs | act)
    std::vector<float*> p_act, p_dy;                         // actor on obs, its gradients
    std::vector<float*> c_act[4], t_act[4], c_dy[4];         // online critics, target critics, critic gradients
    float *pr_w = nullptr, *pr_logp = nullptr, *pr_tgt = nullptr;                                 // probes [B]
    float *pi_part = nullptr, *q_part = nullptr, *h2_part = nullptr; size_t q_part_stride = 0;   // dW partials, head2's gradient
    std::vector<size_t> pi_off, q_off;
    float* scal = nullptr;    // the record values, summed over the updates of one opt
    float* samp = nullptr;    // Policy::sample rows [B][A]
    // host staging of update_on_batch (stage_batch)
    float *u_obs = nullptr, *u_next = nullptr, *u_act = nullptr, *u_rew = nullptr; int8_t *u_term = nullptr, *u_trunc = nullptr; uint64_t u_cap = 0;
    int last_B = 0;

    Self& self() { return static_cast<Self&>(*this); }

    int32_t ensure_batch(int Bn)
    {
        if (Bn <= B) return BDR_OK;
        BDR_HIP(hipStreamSynchronize(stream));
        release(BATCH);
        B = 0;
        const int Kp = pn.L[0].Kp, Kq = qn.L[0].Kp;
        BDR_TRY(alloc(&x_o, (size_t)Bn * Kp, BATCH)); BDR_TRY(alloc(&x_no, (size_t)Bn * Kp, BATCH)); BDR_TRY(alloc(&xq, (size_t)Bn * Kq, BATCH));
        for (auto* vec : {&p_act, &p_dy}) BDR_TRY(layer_bufs(pn, Bn, *vec));
        for (int i = 0; i < NC; ++i) for (auto* vec : {&c_act[i], &t_act[i], &c_dy[i]}) BDR_TRY(layer_bufs(qn, Bn, *vec));
        for (auto p : {&pr_w, &pr_logp, &pr_tgt}) BDR_TRY(alloc(p, Bn, BATCH));
        BDR_TRY(alloc(&pi_part, plan(pn, Bn, pi_off), BATCH));
        q_part_stride = plan(qn, Bn, q_off);
        BDR_TRY(alloc(&q_part, q_part_stride * NC, BATCH));
        BDR_TRY(alloc(&h2_part, (size_t)pad64(A), BATCH));
        BDR_TRY(alloc(&samp, (size_t)Bn * A, BATCH));
        BDR_TRY(self().alloc_batch(Bn));
        B = Bn; batch_gen += 1;
        return BDR_OK;
    }

    // the actor's mean of Bn rows x ([Bn][Kp]) into acts
    int32_t actor_forward(const float* x, std::vector<float*>& acts, int Bn)
    {
        const float* pp[1] = {pi_p}; const float* xs[1] = {x}; std::vector<float*>* as[1] = {&acts};
        return mlp_forward(pn, 1, pp, xs, as, Bn, "pi_fwd");
    }
    // DenseAgent's step from the last layer, under one bracket name, with the critics' tau (the kernel reads it only where targets
    // are tracked)
    int32_t mlp_backward_step(const MlpLayout& net, int nz, float* const* p, float* const* g, float* const* m, float* const* v, float* const* tgt,
                              const float* x0, std::vector<float*>* const* acts, std::vector<float*>* const* dys, float* part, size_t part_stride,
                              const std::vector<size_t>& off, const AdamScalars* sc, int Bn, const char* name, size_t total, const DenseReduceSeg* extra = nullptr)
    {
        return DenseAgent::mlp_backward_step(net, nz, p, g, m, v, tgt, x0, acts, dys, part, part_stride, off, sc, Bn, name, total, cfg.critic_tau,
                                             (int)net.L.size() - 1, extra);
    }
    // the actor's step from dL/dmean (p_dy's last layer) and dL/dhead2 (h2_part): backward and Adam, head2 as one more segment
    int32_t actor_step(int Bn)
    {
        step_pi += 1;
        const AdamScalars sc = opt_scalars(cfg.opt_actor, cfg.lr_actor, step_pi);
        std::vector<float*>* acts[1] = {&p_act}; std::vector<float*>* dys[1] = {&p_dy};
        const DenseReduceSeg h2seg{h2_part, (size_t)pad64(A), 1, (unsigned)(h2_off / 4), (unsigned)(pad64(A) / 4)};
        return mlp_backward_step(pn, 1, &pi_p, &pi_g, &pi_m, &pi_v, nullptr, x_o, acts, dys, pi_part, 0, pi_off, &sc, Bn, "pi_bwd_adam", pi_total, mlp2() ? nullptr : &h2seg);
    }
    // the critics' step from dL/dQ_i (c_dy's last layers): backward, Adam and the soft update of the targets
    int32_t critic_step(int Bn)
    {
        step_q += 1;
        AdamScalars sc[4];
        std::vector<float*>* acts[4]; std::vector<float*>* dys[4];
        for (int i = 0; i < NC; ++i) { sc[i] = opt_scalars(cfg.opt_critic, cfg.lr_critic, step_q); acts[i] = &c_act[i]; dys[i] = &c_dy[i]; }
        return mlp_backward_step(qn, NC, q_p, q_g, q_m, q_v, q_t, xq, acts, dys, q_part, q_part_stride, q_off, sc, Bn, "q_bwd_adam_track", qn.total);
    }
    // the operands of Policy::sample's element code for n rows; in train mode without host draws it takes the next n * A draws of the
    // device stream (the layer path and the fused kernel advance the same counter: their calls can be interleaved)
    SampleElem sample_elem(int n, const float* z)
    {
        SampleElem e{};
        e.head2 = pi_p + h2_off; e.mlp2 = mlp2() ? 1 : 0;
        e.lo = (float)cfg.min_log_std; e.hi = (float)cfg.max_log_std; e.tanh_limit = cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
        e.amin = (float)cfg.action_min; e.amax = (float)cfg.action_max; e.scale = (float)cfg.action_scale;
        e.train = train ? 1 : 0; e.seed = cfg.seed; e.z = z;
        if (train && !z) { e.counter = noise_counter; noise_counter += (uint64_t)n * A; }
        return e;
    }
    // Policy::sample of n rows from the actor's last layer (mean) into out, and into the action columns of the critic input xqd when
    // given: host draws z, else in train mode the device stream
    int32_t sample_pack(const float* mean, int n, const float* z, float* out, float* xqd, const char* name)
    {
        CandleSampleArgs p{};
        p.mean = mean; p.ldm = pn.L.back().Np; p.A = A; p.n = n;
        p.e = sample_elem(n, z);
        p.out = out; p.xq = xqd; p.ldq = qn.L[0].Kp; p.O = O;
        const int tot = n * A;
        Bracket br(this, name);
        BDR_HIP(step_launch(stream, true, k_candle_sample, dim3((tot + 255) / 256), dim3(256), p));
        return BDR_OK;
    }

    // ---- update_on_batch ----
    // host rows -> the staging buffers, grown on demand (with the agent's own: alloc_staging)
    int32_t stage_batch(uint64_t n, const float* obs, const float* act, const float* next_obs, const float* reward, const int8_t* term, const int8_t* trunc)
    {
        BDR_HIP(hipSetDevice(device));
        BDR_TRY(ensure_batch((int)n));
        if (n > u_cap) {
            BDR_HIP(hipStreamSynchronize(stream));
            release(STAGING);
            u_cap = 0;
            BDR_TRY(alloc(&u_obs, n * O, STAGING, false)); BDR_TRY(alloc(&u_next, n * O, STAGING, false));
            BDR_TRY(alloc(&u_act, n * A, STAGING, false)); BDR_TRY(alloc(&u_rew, n, STAGING, false));
            BDR_TRY(alloc(&u_term, round_up(n, 16), STAGING, false)); BDR_TRY(alloc(&u_trunc, round_up(n, 16), STAGING, false));
            BDR_TRY(self().alloc_staging(n));
            u_cap = n;
        }
        BDR_HIP(hipMemcpyAsync(u_obs, obs, n * O * 4, hipMemcpyHostToDevice, stream));
        BDR_HIP(hipMemcpyAsync(u_next, next_obs, n * O * 4, hipMemcpyHostToDevice, stream));
        BDR_HIP(hipMemcpyAsync(u_act, act, n * A * 4, hipMemcpyHostToDevice, stream));
        BDR_HIP(hipMemcpyAsync(u_rew, reward, n * 4, hipMemcpyHostToDevice, stream));
        BDR_HIP(hipMemcpyAsync(u_term, term, n, hipMemcpyHostToDevice, stream));
        BDR_HIP(hipMemcpyAsync(u_trunc, trunc, n, hipMemcpyHostToDevice, stream));
        return BDR_OK;
    }
    // after the update: the profile, the record values (rec: N_RECORD floats, or null) and the device's error words
    int32_t batch_done(float* rec)
    {
        prof_collect(this);
        if (rec) BDR_HIP(hipMemcpyAsync(rec, scal, Self::N_RECORD * 4, hipMemcpyDeviceToHost, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        return err_check();
    }

    // ---- agent plumbing ----
    int32_t opt(bdr_replay* r) override
    {
        BDR_TRY(check_replay(r, Self::NAME));
        const int Bn = (int)cfg.batch_size;
        BDR_TRY(ensure_batch(Bn));
        for (uint64_t u = 0; u < cfg.n_updates_per_opt; ++u) {
            { Bracket br(this, "sample"); BDR_TRY(replay_sample_on_stream(r, Bn, stream)); }
            BDR_TRY(self().update(Bn, (const float*)r->b_obs, (const float*)r->b_act, (const float*)r->b_next, r->b_reward, r->b_term, r->b_trunc, u == 0));
        }
        return BDR_OK;
    }
    int32_t noise(float* dev, size_t n) override   // the N(0,1) stream of Policy::sample in train mode
    {
        BDR_HIP(step_launch(stream, true, k_candle_randn, dim3((unsigned)((n + 255) / 256)), dim3(256), dev, n, cfg.seed, noise_counter));
        noise_counter += n;
        return BDR_OK;
    }

    // Policy::sample (util/actor.rs:226-241) of n observation rows (host rows, or device rows inside sample_device); out: [n][A]
    int32_t sample(uint64_t n, const float* obs, float* act_out)
    {
        BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
        if (act_fused_on()) return act_fused(nullptr, n, obs, BDR_DTYPE_F32, obs_rows_on_device, obs_rows_on_device ? obs_row_stride : (uint64_t)O * 4, act_out, nullptr);
        BDR_HIP(hipSetDevice(device));
        BDR_TRY(ensure_batch((int)n));
        int32_t st = pack_acting_obs(obs, n, x_o, pn.L[0].Kp);
        if (st == BDR_OK) st = actor_forward(x_o, p_act, (int)n);
        if (st == BDR_OK) st = sample_pack(p_act.back(), (int)n, nullptr, samp, nullptr, "sample_pack");
        if (st == BDR_OK) st = rows_to_host(samp, act_out, n * A);
        slot_cursor = 0;
        return st;
    }
    int32_t sample_device(uint64_t n, const void* obs_dev, uint64_t row_stride, float* act_out)
    {
        return with_device_rows(obs_dev, row_stride, [&](const float* rows) { return sample(n, rows, act_out); });
    }
    // ---- DenseAgent's acting hooks (dense_agent.hpp) ----
    const MlpLayout& act_net() const override { return pn; }
    const float* act_params() const override { return pi_p; }
    int32_t act_check_out(const float* act_out, const int64_t*) const override
    {
        BDR_REQUIRE(act_out, "null argument");
        return BDR_OK;
    }
    int32_t act_epilogue(DenseActArgs& a, uint64_t n) override
    {
        BDR_TRY(ensure_batch((int)n));
        a.mode = DA_CANDLE; a.e = sample_elem((int)n, nullptr); a.out = samp;
        return BDR_OK;
    }
    int32_t act_results(uint64_t n, float* act_out, int64_t*) override { return rows_to_host(samp, act_out, n * A); }
    int32_t act_layers(uint64_t n, const void* rows, bool on_device, uint64_t stride, float* act_out, int64_t*) override
    {
        return on_device ? sample_device(n, rows, stride, act_out) : sample(n, static_cast<const float*>(rows), act_out);
    }
    bool sample_f32(uint64_t n, const void* obs, bool on_device, uint64_t stride, float* act, int32_t* st) override
    {
        *st = !obs || !act ? fail(BDR_ERR_INVALID, "null argument")
            : on_device ? sample_device(n, obs, stride, act) : sample(n, static_cast<const float*>(obs), act);
        return true;
    }

    // ---- parameter views ----
    // which: 0 actor, 1+i critic_i, 1+NC+i critic_tgt_i, then the agent's own models from 1+2NC (own_view);  +100 grad, +200 exp_avg,
    // +300 exp_avg_sq
    bool param_view(int which, ParamView* pv) override
    {
        const int role = which / 100, id = which % 100;
        if (role > 3 || which < 0) return false;
        if (id == 0) { float* r[4] = {pi_p, pi_g, pi_m, pi_v}; *pv = actor_view(r[role]); return true; }
        if (id >= 1 && id <= NC) { const int i = id - 1; float* r[4] = {q_p[i], q_g[i], q_m[i], q_v[i]}; *pv = mlp_view(qn, r[role]); return true; }
        if (id >= 1 + NC && id <= 2 * NC) { if (role == 0) *pv = mlp_view(qn, q_t[id - 1 - NC]); return role == 0; }
        return self().own_view(id - 1 - 2 * NC, role, pv);
    }
    // Mlp2's heads in the actor's reference view: the last layer's [weight [2A][H] | bias [2A]] (mean rows, then std rows) <->
    // mean.weight [A][H], mean.bias [A], std.weight [A][H], std.bias [A] (mlp2.rs:47-52)
    void mlp2_heads(float* ref, bool to_reference) const
    {
        const size_t H = (size_t)pn.L.back().in, a = (size_t)A, nw = a * H;
        float* t = ref + pn.ref_total - (2 * nw + 2 * a);
        std::vector<float> o(t, t + 2 * nw + 2 * a);
        // layer order: Wm Ws bm bs; reference order: Wm bm Ws bs - the two middle blocks change places
        if (to_reference) { std::copy(o.begin() + 2 * nw, o.begin() + 2 * nw + a, t + nw); std::copy(o.begin() + nw, o.begin() + 2 * nw, t + nw + a); }
        else { std::copy(o.begin() + nw + a, o.begin() + 2 * nw + a, t + nw); std::copy(o.begin() + nw, o.begin() + nw + a, t + 2 * nw); }
    }
    // the actor: pn's layers, then Mlp3's head2 [A] behind them (Mlp2: its two heads reordered, no head2)
    ParamView actor_view(float* arena)
    {
        ParamView v = mlp_view(pn, arena, pi_total);
        if (mlp2()) {
            v.to_reference = [this](const float* in, float* ref) { mlp_to_reference(pn, 0, in, ref); mlp2_heads(ref, true); };
            v.from_reference = [this](const float* ref, float* in) {
                std::vector<float> r(ref, ref + pn.ref_total);
                mlp2_heads(r.data(), false);
                mlp_to_internal(pn, 0, r.data(), in);
            };
            return v;
        }
        v.count = pn.ref_total + (uint64_t)A;
        v.to_reference = [this](const float* in, float* ref) { mlp_to_reference(pn, 0, in, ref); std::copy(in + h2_off, in + h2_off + A, ref + pn.ref_total); };
        v.from_reference = [this](const float* ref, float* in) { mlp_to_internal(pn, 0, ref, in); std::copy(ref + pn.ref_total, ref + pn.ref_total + A, in + h2_off); };
        return v;
    }

    // ---- checkpoints: actor.pt, critic.pt, critic.tgt.pt ----
    static void mlp_meta(const MlpLayout& net, const std::string& prefix, std::vector<NamedTensor>& mt) { candle::mlp_meta(net, prefix, mt); }
    std::vector<NamedTensor> actor_meta() const
    {
        std::vector<NamedTensor> mt;
        mlp_meta(pn, "actor.", mt);
        if (mlp2()) {   // mlp2.rs:47-52: the trunk's ln{i}, then the heads `mean` and `std`
            mt.resize(mt.size() - 2);
            const uint64_t H = (uint64_t)pn.L.back().in;
            for (const char* h : {"mean", "std"}) {
                mt.push_back({std::string("actor.") + h + ".weight", {(uint64_t)A, H}});
                mt.push_back({std::string("actor.") + h + ".bias", {(uint64_t)A}});
            }
        } else mt.push_back({"actor.head2", {1, (uint64_t)A}});
        return mt;
    }
    std::vector<NamedTensor> critic_meta() const   // one VarMap holds every critic: critic{i}.mlp.ln{k}.* (util/critic.rs:155-170)
    {
        std::vector<NamedTensor> mt;
        for (int i = 0; i < NC; ++i) mlp_meta(qn, "critic" + std::to_string(i) + ".", mt);
        return mt;
    }
    // actor, critic, critic.tgt - critic.tgt is saved from, and loaded into, the ONLINE critics: MultiCritic::save / load (util/critic.rs:272-298)
    // put both files through the online critics' VarMap, the second load wins and the targets stay as they are - then the agent's own files
    void checkpoint_files(std::vector<CheckpointFile>& files) override
    {
        std::vector<int> critics;
        for (int i = 0; i < NC; ++i) critics.push_back(1 + i);
        files = {{"actor", actor_meta(), {0}, {0}}, {"critic", critic_meta(), critics, critics}, {"critic.tgt", critic_meta(), critics, critics}};
        self().own_files(files);
    }

    // ---- group copies and hyperparameters (dense_agent.hpp): the actor's and critics', then the agent's own (own_arenas, own_steps, own_hyper) ----
    void state_arenas(std::vector<StateArena>& out) override
    {
        out = {{pi_p, pi_total}, {pi_g, pi_total}, {pi_m, pi_total}, {pi_v, pi_total}};
        for (int i = 0; i < NC; ++i)
            for (float* a : {q_p[i], q_t[i], q_g[i], q_m[i], q_v[i]}) out.push_back({a, qn.total});
        self().own_arenas(out);
    }
    void adopt_steps(const DenseAgent& src) override
    {
        const Self& s = static_cast<const Self&>(src);
        step_pi = s.step_pi; step_q = s.step_q;
        self().own_steps(s);
    }
    double* hyper_field(int32_t id) override
    {
        if (id >= BDR_HYPER_LR_ACTOR && id <= BDR_HYPER_ACTOR_WEIGHT_DECAY) return opt_field(cfg.opt_actor, cfg.lr_actor, id - BDR_HYPER_LR_ACTOR);
        if (id >= BDR_HYPER_LR_CRITIC && id <= BDR_HYPER_CRITIC_WEIGHT_DECAY) return opt_field(cfg.opt_critic, cfg.lr_critic, id - BDR_HYPER_LR_CRITIC);
        if (id == BDR_HYPER_GAMMA) return &cfg.gamma;
        if (id == BDR_HYPER_CRITIC_TAU) return &cfg.critic_tau;
        return self().own_hyper(id);
    }

    // ---- hooks an agent may replace ----
    int32_t init_own() { return BDR_OK; }                       // create: the agent's own models, after the actor's and critics'
    int32_t alloc_staging(uint64_t) { return BDR_OK; }          // stage_batch: the agent's own staging rows (alloc(..., STAGING))
    bool own_view(int /*k*/, int /*role*/, ParamView*) { return false; }   // model 1 + 2NC + k
    void own_files(std::vector<CheckpointFile>&) {}             // checkpoint files behind the core's three
    void own_arenas(std::vector<StateArena>&) {}                // state_arenas: the arenas of the agent's own models
    void own_steps(const Self&) {}                              // adopt_steps: the step counters of the agent's own models
    double* own_hyper(int32_t) { return nullptr; }              // hyper_field: the agent's own hyperparameters

    // bdr_*_create after its null check: the checks in their order, the device, then the agent with its initial parameters.
    // value / opt_value: IQL's value model, checked before the actor's; one_row: why a one-row batch is refused (AWAC), null where one
    // row is allowed.
    // actor_kind: BDR_ACTOR_MLP3 for IQL and AWAC; SAC passes its config's.
    static int32_t create(const Cfg& c, bdr_agent** out, const bdr_mlp_config* value, const bdr_adamw_config* opt_value, const char* one_row,
                          int32_t actor_kind = BDR_ACTOR_MLP3)
    {
        BDR_REQUIRE(c.device >= 0, "No device is given for %s agent", Self::NAME);
        BDR_REQUIRE(c.obs_dim >= 1 && c.obs_dim <= 4096 && c.act_dim >= 1 && c.act_dim <= 256, "bad obs/act dims");
        if (value) BDR_TRY(check_mlp(*value, "value", false));
        BDR_REQUIRE(actor_kind == BDR_ACTOR_MLP3 || actor_kind == BDR_ACTOR_MLP2, "unknown actor_kind %d (BDR_ACTOR_MLP3 or BDR_ACTOR_MLP2)", actor_kind);
        const bool two = actor_kind == BDR_ACTOR_MLP2;
        BDR_TRY(check_mlp(c.actor, two ? "actor (Mlp2)" : "actor (Mlp3)", true));
        // mlp.rs:14-24: mlp_forward's loop bound 0..=n_layers-2 underflows (usize) with a single trunk layer
        BDR_REQUIRE(!two || c.actor.n_units >= 2, "actor (Mlp2): the reference's trunk needs at least 2 layers (units), got %d", c.actor.n_units);
        BDR_TRY(check_mlp(c.critic, "critic", false));
        BDR_REQUIRE(c.n_critics >= 1 && c.n_critics <= 4, "n_critics must be in [1,4]");
        if (one_row) BDR_REQUIRE(c.batch_size != 1, "%s", one_row);
        BDR_REQUIRE(c.batch_size >= 1 && c.batch_size <= 65536 && c.n_updates_per_opt >= 1, "bad batch / update counts");
        BDR_REQUIRE(c.action_limit == BDR_ACTION_LIMIT_CLAMP || c.action_limit == BDR_ACTION_LIMIT_TANH, "unknown action limit");
        BDR_REQUIRE(c.critic_loss == BDR_LOSS_MSE || c.critic_loss == BDR_LOSS_SMOOTH_L1, "unknown critic loss");
        if (opt_value) BDR_TRY(check_opt(*opt_value, "value"));
        BDR_TRY(check_opt(c.opt_actor, "actor")); BDR_TRY(check_opt(c.opt_critic, "critic"));
        BDR_TRY(ensure_device(c.device));
        Self* a = new Self();
        a->cfg = c; a->device = c.device; a->train = c.train != 0;
        a->O = c.obs_dim; a->A = c.act_dim; a->NC = c.n_critics;
        a->actor_kind = actor_kind;
        // Mlp3: no output activation.  Mlp2: ReLU after every trunk layer, then the two heads as one layer [mean | s] without one
        a->pn = make_mlp(a->O, c.actor.units, c.actor.n_units, two ? 2 * a->A : a->A, false);
        a->qn = make_mlp(a->O + a->A, c.critic.units, c.critic.n_units, 1, c.critic.activation_out == BDR_ACTIVATION_RELU);
        a->h2_off = a->pn.total; a->pi_total = a->pn.total + (two ? 0 : (size_t)pad64(a->A));
        const int32_t st = [&]() -> int32_t {
            BDR_HIP(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
            BDR_TRY(a->err_init());
            for (auto p : {&a->pi_p, &a->pi_g, &a->pi_m, &a->pi_v}) BDR_TRY(a->alloc(p, a->pi_total, AGENT));
            for (int i = 0; i < a->NC; ++i)
                for (auto p : {&a->q_p[i], &a->q_t[i], &a->q_g[i], &a->q_m[i], &a->q_v[i]}) BDR_TRY(a->alloc(p, a->qn.total, AGENT));
            BDR_TRY(a->alloc(&a->scal, Self::N_RECORD, AGENT));
            // initial parameters: the library's initialiser, head2 = 0 (mlp3.rs: Init::Const(0.)); targets are copies of the critics
            std::vector<float> ref(a->param_count(0), 0.f);
            mlp_init_reference(a->pn, c.seed * 7 + 1, ref.data());
            BDR_TRY(a->set_params(0, ref.data(), ref.size()));
            ref.assign(a->qn.ref_total, 0.f);
            for (int i = 0; i < a->NC; ++i) {
                mlp_init_reference(a->qn, c.seed * 7 + 2 + i, ref.data());
                BDR_TRY(a->set_params(1 + i, ref.data(), ref.size()));
                BDR_TRY(a->set_params(1 + a->NC + i, ref.data(), ref.size()));
            }
            BDR_TRY(a->init_own());
            return a->ensure_batch((int)c.batch_size);
        }();
        if (st != BDR_OK) { delete a; return st; }
        *out = a;
        return BDR_OK;
    }
};

}  // namespace
