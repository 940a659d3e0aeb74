// DQN agent of border-candle-agent on MI355X (border-candle-agent/src/dqn/{base.rs,config.rs,explorer.rs,model.rs}) with an Mlp
// Q-network (mlp/base.rs, mlp.rs:14-24: ReLU after every layer but the last, activation_out after the last).  Not the tch Dqn of
// mlp_agents.hip / dqn.hip: this one has the reference's SmallRng exploration stream, candle's optimizers, safetensors checkpoints
// (qnet.pt, qnet_tgt.pt) and sits on DenseAgent (dense_agent.hpp) like BC, so it has bdr_agent_sample_raw, k_dense_act and the
// DenseAgent checkpoint helpers.  Hidden layers, the grouped weight gradient and the fused reduce + Adam (+ soft update) are
// dense.hpp's FP32-MFMA kernels, unchanged.  This file holds the agent's three kernels, its update schedule, its record, Policy::sample
// with the host-side explorer, and its entry points.
//   k_cdqn_pack  obs and next_obs into the padded first-layer inputs, one launch
//   k_cdqn_td    Dqn::update_critic (dqn/base.rs:59-170) behind the forward passes: gather, first-maximum argmax, gather, the TD
//                target, the loss element and dLoss/dpred into the last layer's padded gradient rows, the record's means
//   k_cdqn_act   Policy::sample's device part on the layer path: the Q rows [n][A] and each row's first maximum
// One update: pack, L forwards (the passes (p, obs), (p_tgt, next_obs) and, double_dqn, (p, next_obs) share each layer's launch),
// k_cdqn_td, L - 1 input gradients, the grouped dW, reduce + Adam: 2 L + 3 launches, 9 at the CartPole shape (L = 3), plus the
// ring's gather.  The soft update rides in the reduce + Adam launch of the opt's last update on the opts that track (dqn/base.rs:180-184).
// Every sum has one order (candle::row_sum), so an update gives the same bits run to run and agent to agent.
#include <algorithm>
#include <cstdlib>
#include <deque>

#include "candle_actor.hpp"

using namespace bdr;

namespace {

// obs, next_obs [B][O] -> the zero-padded first-layer inputs x_o, x_no [B][Kp] in one launch (the padding columns were zeroed when
// the buffers were allocated and are never written).  Bounds: t < B O; row b < B, column c < O <= Kp.
__global__ __launch_bounds__(256) void k_cdqn_pack(const float* __restrict__ obs, const float* __restrict__ next_obs, int O, int Kp, int B,
                                                   float* __restrict__ x_o, float* __restrict__ x_no)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * O) return;
    const size_t d = (size_t)(t / O) * Kp + t % O;
    x_o[d] = obs[t];
    x_no[d] = next_obs[t];
}

// ---- k_cdqn_td --------------------------------------------------------------------------------------------------------------------
// One 1024-thread workgroup; thread t owns rows t, t + 1024, ...
//   pred[b]   = Q(obs)[b][act[b]]                                                   (dqn/base.rs:80-86)
//   y[b]      = argmax_j Q(next_obs)[b][j] of the ONLINE net (double_dqn) or of the target net, the first maximum (:101-108)
//   q_next[b] = Q_tgt(next_obs)[b][y[b]]
//   tgt[b]    = reward + (((1 - is_terminated) * gamma) * q_next), every operation rounded to f32 (td_target; :113)
//   l, g      = candle::critic_loss_elem(pred - tgt)  (mse / smooth_l1, util.rs:144-152);  dpred = g / B
//   dy[b][:]  = the WHOLE padded row of the last layer's output gradient: dpred in column act[b] - zero where the Mlp has an output
//               ReLU and it is closed (pred <= 0) - and zero elsewhere
//   scal[0] = mean l; with `verbose`: scal[1..4] = the means of pred, reward, tgt, tgt - pred (:88-133), in candle::row_sum's order.
// An action outside [0, A) raises err[ERR_ACTION] - the reduce + Adam launch of this update reads the word and leaves the parameters
// alone - and is clamped for the reads and writes here.
// Bounds.  Reads: q_on / q_tg / q_on_next rows b < B, columns j < A, row stride Np; act, reward, term at b < B.  Writes: dy rows
// b < B, columns j < Np (the row stride); pred / q_next / y / tgt / dpred / lrow at b < B; scal[0..4]; err[ERR_ACTION].  A thread
// whose row index is >= B touches nothing.  LDS: red[32].
// Cost.  ONE workgroup writes all B x Np gradient elements and walks the rows 1024 at a time: a few microseconds at the shapes the
// agent is built for (CartPole: 64 x 64; an Atari-sized head: 256 x 64), but serial in B x Np - at the limits the constructor
// accepts (B 65536, 4096 actions: 2^28 elements) this launch, not the GEMMs, would bound the update.  Nothing that large was measured.
struct CdqnTdArgs {
    const float* q_on; const float* q_tg; const float* q_on_next;   // [B][Np]; q_on_next null without double_dqn
    int Np, A, B;
    const uint8_t* act; int act_bytes;                              // one i64 per row
    const float* reward; const int8_t* term;
    float gamma; int loss_kind, relu_out, verbose;
    float* dy;                                                      // [B][Np]
    float *pred, *q_next, *y, *tgt, *dpred, *lrow;                  // [B]
    float* scal; unsigned* err;
};
__device__ __forceinline__ long long cdqn_action(const CdqnTdArgs& p, int b, bool* bad)
{
    long long a = *reinterpret_cast<const long long*>(p.act + (size_t)b * p.act_bytes);
    *bad = a < 0 || a >= p.A;
    if (*bad) a = a < 0 ? 0 : p.A - 1;
    return a;
}
__global__ __launch_bounds__(1024) void k_cdqn_td(CdqnTdArgs p)
{
    __shared__ float red[32];
    const float invB = 1.0f / (float)p.B;
    for (int b = threadIdx.x; b < p.B; b += 1024) {
#pragma clang fp contract(off)
        bool bad;
        const long long a = cdqn_action(p, b, &bad);
        if (bad) atomicOr(p.err + bdr_agent::ERR_ACTION, 1u);
        const size_t row = (size_t)b * p.Np;
        const float pred = p.q_on[row + a];
        const int y = dqn_q_argmax((p.q_on_next ? p.q_on_next : p.q_tg) + row, p.A);
        const float qn = p.q_tg[row + y];
        const float nt = (float)(1 - (int)p.term[b]);
        const float tgt = td_target(p.reward[b], nt, p.gamma, qn);
        const float d = pred - tgt;
        float l, g;
        candle::critic_loss_elem(p.loss_kind, d, l, g);
        const float gp = g * invB;
        p.pred[b] = pred; p.q_next[b] = qn; p.y[b] = (float)y; p.tgt[b] = tgt; p.dpred[b] = gp; p.lrow[b] = l;
    }
    __syncthreads();   // the rows' dpred, written above by other threads of this workgroup, are read below
    const unsigned n_dy = (unsigned)p.B * (unsigned)p.Np;   // <= 65536 x 4096 = 2^28 (cdqn_check): 32-bit index arithmetic
    for (unsigned e = threadIdx.x; e < n_dy; e += 1024) {
        const int b = (int)(e / (unsigned)p.Np), j = (int)(e % (unsigned)p.Np);
        bool bad;
        const long long a = cdqn_action(p, b, &bad);
        const bool open = !p.relu_out || p.pred[b] > 0.f;   // the Mlp's output ReLU: no gradient where it is closed
        p.dy[e] = j == (int)a && open ? p.dpred[b] : 0.f;
    }
    // (row_sum reads row b in the thread that wrote it: b = base + threadIdx.x in both loops)
    const float sl = candle::row_sum(p.B, [&](int b) { return p.lrow[b]; }, red);
    if (threadIdx.x == 0) p.scal[0] = candle::acc(0.f, sl, invB);
    if (!p.verbose) return;
    const float sp = candle::row_sum(p.B, [&](int b) { return p.pred[b]; }, red);
    const float sr = candle::row_sum(p.B, [&](int b) { return p.reward[b]; }, red);
    const float st = candle::row_sum(p.B, [&](int b) { return p.tgt[b]; }, red);
    const float sd = candle::row_sum(p.B, [&](int b) {
#pragma clang fp contract(off)
        return p.tgt[b] - p.pred[b];
    }, red);
    if (threadIdx.x == 0) {
        p.scal[1] = candle::acc(0.f, sp, invB); p.scal[2] = candle::acc(0.f, sr, invB);
        p.scal[3] = candle::acc(0.f, st, invB); p.scal[4] = candle::acc(0.f, sd, invB);
    }
}

// Policy::sample's device part on the layer path (dqn/base.rs:203, :226) from the last layer's output z [n][ld]: q [n][A] = the
// rows without their padding, idx [n] = dqn_q_argmax of each row - the values and the rule of k_dense_act's DA_DQN epilogue.
// Bounds: rows b < n, columns j < A <= ld.
struct CdqnActArgs { const float* z; int ld, A, n; float* q; long long* idx; };
__global__ __launch_bounds__(256) void k_cdqn_act(CdqnActArgs p)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < p.n * p.A) p.q[t] = p.z[(size_t)(t / p.A) * p.ld + t % p.A];
    if (t < p.n) p.idx[t] = dqn_q_argmax(p.z + (size_t)t * p.ld, p.A);
}

// ---- the exploration stream -------------------------------------------------------------------------------------------------------
// rand 0.8.5's SmallRng on 64-bit targets as Dqn uses it (dqn/base.rs:274 `SmallRng::seed_from_u64(42)`, explorer.rs), restated from
// rand's source; nothing here can run rand, so every rule below is unpinned until tools/upstream_kat has run.  The
// numpy restatement of the same rules is tests/candle_dqn_restatement.py's SmallRng.
struct SmallRng {
    uint64_t s[4] = {0, 0, 0, 0};
    // rule 1 + 2: the 32 seed bytes of rand_core's default SeedableRng::seed_from_u64 (the PCG32 fill that also makes the ring's
    // ChaCha key: chacha.hpp) read as four little-endian u64.  (rand 0.8.5's SmallRng wrapper does not forward to xoshiro's own
    // SplitMix64 seed_from_u64.)
    void seed_from_u64(uint64_t seed)
    {
        uint32_t k[8];
        bdr::seed_from_u64(seed, k);
        for (int i = 0; i < 4; ++i) s[i] = (uint64_t)k[2 * i] | ((uint64_t)k[2 * i + 1] << 32);
    }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    // rule 3: xoshiro256++ 1.0
    uint64_t next_u64()
    {
        const uint64_t r = rotl(s[0] + s[3], 23) + s[0];
        const uint64_t t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
        s[2] ^= t;
        s[3] = rotl(s[3], 45);
        return r;
    }
    uint32_t next_u32() { return (uint32_t)(next_u64() >> 32); }                       // rule 4
    float gen_f32() { return (float)(next_u32() >> 8) * (1.0f / 16777216.0f); }        // rule 5: 24 bits, [0, 1)
    static uint64_t range_zone(uint64_t A) { return (A << __builtin_clzll(A)) - 1; }   // rule 6: UniformInt<i64>::sample_single
    int64_t gen_range(uint64_t A)
    {
        const uint64_t zone = range_zone(A);
        for (;;) {
            const unsigned __int128 m = (unsigned __int128)next_u64() * A;
            if ((uint64_t)m <= zone) return (int64_t)(uint64_t)(m >> 64);
        }
    }
    // rule 7: WeightedIndex<f32>::new(w) then sample.  false: a weight that is not >= 0, or a total of 0 (the reference panics on
    // the unwrap of InvalidWeight / AllWeightsZero).  cum: scratch of n - 1 floats.
    bool weighted_index(const float* w, int n, float* cum, int* out)
    {
        if (!(w[0] >= 0.f)) return false;
        float total = w[0];
        for (int i = 1; i < n; ++i) {
            if (!(w[i] >= 0.f)) return false;
            cum[i - 1] = total;
            total = total + w[i];
        }
        if (total == 0.f) return false;
        if (!(total <= 3.402823466e+38f)) return false;   // (Uniform::new panics on a non-finite range)
        // UniformFloat<f32>::new(0, total): scale = total - 0, stepped one ulp down while scale * max_rand + 0 >= total
        const float max_rand = 1.0f - 1.1920928955078125e-07f;
        float scale = total;
        while (mul(scale, max_rand) >= total) {
            uint32_t bits; memcpy(&bits, &scale, 4); bits -= 1; memcpy(&scale, &bits, 4);
        }
        const float u = (float)(next_u32() >> 9) * (1.0f / 8388608.0f);   // value1_2 - 1.0: 23 bits, [0, 1)
        const float chosen = mul(u, scale);                                // (+ low, which is 0)
        int k = 0;   // partition_point(|w| w <= chosen)
        while (k < n - 1 && cum[k] <= chosen) ++k;
        *out = k;
        return true;
    }
    static float mul(float a, float b) { volatile float r = a * b; return r; }   // one f32 product, no wider intermediate
    // rule 8: a softmax row in f32 (candle_nn::ops::softmax): e_j = exp(q_j - max), s = sum e_j in index order, p_j = e_j / s
    static void softmax_row(const float* q, int n, float* p)
    {
        float mx = q[0];
        for (int j = 1; j < n; ++j) mx = q[j] > mx ? q[j] : mx;
        float s = 0.f;
        for (int j = 0; j < n; ++j) { p[j] = expf(q[j] - mx); s = s + p[j]; }
        for (int j = 0; j < n; ++j) p[j] = p[j] / s;
    }
};

}  // namespace

// ================================================================================================
// The buffer lifetimes, the layer-by-layer forward, the backward step, the observation rows of an acting call and the reference
// layout are DenseAgent's (dense_agent.hpp); the candle DQN adds its two parameter sets, its schedule, its record and its sample.
struct CandleDqn : DenseAgent {
    bdr_candle_dqn_config cfg;
    MlpLayout net;                     // one layout for qnet and qnet_tgt
    float *p = nullptr, *p_tgt = nullptr, *g = nullptr, *m = nullptr, *v = nullptr;   // arenas
    uint64_t step = 0, soft_update_counter = 0;
    // host counters as they stood BEFORE the opt each enqueued update belongs to, by Adam step number (settle)
    struct Mark { uint64_t step, n_opts, soft; };
    std::deque<Mark> marks; uint64_t opt_n0 = 0, opt_s0 = 0;
    unsigned long long* applied = nullptr;   // device: the Adam step number of the last reduce + Adam launch that was not skipped
    SmallRng rng;
    // batch buffers
    int B = 0;
    float *x_o = nullptr, *x_no = nullptr;                 // [B][Kp] padded obs, next_obs
    std::vector<float*> a_on, a_tg, a_onn, dy;             // activations of (p, obs), (p_tgt, next_obs), (p, next_obs); gradients
    float *pr_pred = nullptr, *pr_qn = nullptr, *pr_y = nullptr, *pr_tgt = nullptr, *pr_dpred = nullptr, *lrow = nullptr;   // [B]
    float* part = nullptr; std::vector<size_t> off;
    float* samp = nullptr; long long* samp_idx = nullptr;  // Policy::sample: Q rows [B][A], first-maximum indices [B]
    float* scal = nullptr;                                 // loss, pred_mean, reward_mean, tgt_mean, tgt_minus_pred_mean
    // staging of update_on_batch
    float *u_obs = nullptr, *u_next = nullptr, *u_rew = nullptr; long long* u_act = nullptr; int8_t* u_term = nullptr; uint64_t u_cap = 0;
    int last_B = 0;
    // the acting call in progress: what it copies back, and where
    bool q_mode = false;                                   // bdr_agent_qvalues: the Q rows whatever the explorer is
    std::vector<float> h_q; std::vector<int64_t> h_idx;

    bool verbose() const { return cfg.record_verbose_level >= 2; }

    int32_t ensure_batch(int Bn)
    {
        if (Bn <= B) return BDR_OK;
        BDR_HIP(hipStreamSynchronize(stream));
        release(BATCH);
        B = 0;
        BDR_TRY(alloc(&x_o, (size_t)Bn * net.L[0].Kp, BATCH)); BDR_TRY(alloc(&x_no, (size_t)Bn * net.L[0].Kp, BATCH));
        for (auto* vec : {&a_on, &a_tg, &a_onn, &dy}) BDR_TRY(layer_bufs(net, Bn, *vec));
        for (auto q : {&pr_pred, &pr_qn, &pr_y, &pr_tgt, &pr_dpred, &lrow}) BDR_TRY(alloc(q, Bn, BATCH));
        BDR_TRY(alloc(&part, plan(net, Bn, off), BATCH));
        BDR_TRY(alloc(&samp, (size_t)Bn * A, BATCH));
        BDR_TRY(alloc(&samp_idx, Bn, BATCH));
        B = Bn;
        return BDR_OK;
    }

    // Dqn::update_critic (dqn/base.rs:59-170) on device-resident rows; track: the soft update of opt_ (:180-184) rides in this
    // update's reduce + Adam launch
    int32_t update(int Bn, const float* obs, const uint8_t* act, int act_bytes, const float* next_obs, const float* reward, const int8_t* term, bool track)
    {
        BDR_TRY(ensure_batch(Bn));
        const int L = (int)net.L.size();
        const DenseLayer& last = net.L[L - 1];
        {
            Bracket br(this, "pack");
            BDR_HIP(step_launch(stream, false, k_cdqn_pack, dim3((unsigned)((Bn * O + 255) / 256)), dim3(256), obs, next_obs, O, net.L[0].Kp, Bn, x_o, x_no));
        }
        {
            const float* pp[3] = {p, p_tgt, p}; const float* xs[3] = {x_o, x_no, x_no}; std::vector<float*>* as[3] = {&a_on, &a_tg, &a_onn};
            BDR_TRY(mlp_forward(net, cfg.double_dqn ? 3 : 2, pp, xs, as, Bn, "fwd"));
        }
        {
            CdqnTdArgs t{};
            t.q_on = a_on[L - 1]; t.q_tg = a_tg[L - 1]; t.q_on_next = cfg.double_dqn ? a_onn[L - 1] : nullptr;
            t.Np = last.Np; t.A = A; t.B = Bn; t.act = act; t.act_bytes = act_bytes; t.reward = reward; t.term = term;
            t.gamma = (float)cfg.discount_factor; t.loss_kind = cfg.critic_loss; t.relu_out = last.relu; t.verbose = verbose() ? 1 : 0;
            t.dy = dy[L - 1]; t.pred = pr_pred; t.q_next = pr_qn; t.y = pr_y; t.tgt = pr_tgt; t.dpred = pr_dpred; t.lrow = lrow;
            t.scal = scal; t.err = dev_err;
            Bracket br(this, "cdqn_td");
            BDR_HIP(step_launch(stream, false, k_cdqn_td, dim3(1), dim3(1024), t));
        }
        step += 1;
        marks.push_back(Mark{step, opt_n0, opt_s0});
        if (marks.size() > 4096) marks.pop_front();
        const AdamScalars sc = opt_scalars(cfg.opt, cfg.lr, step);
        std::vector<float*>* acts[1] = {&a_on}; std::vector<float*>* dys[1] = {&dy};
        float* tg[1] = {p_tgt};
        BDR_TRY(mlp_backward_step(net, 1, &p, &g, &m, &v, track ? tg : nullptr, x_o, acts, dys, part, 0, off, &sc, Bn, {"dx", "dw", "reduce_adam"}, net.total,
                                  cfg.tau, L - 1, nullptr, dev_err + ERR_ACTION, applied, step));
        last_B = Bn;
        return BDR_OK;
    }
    // opt_'s bookkeeping before its last update (dqn/base.rs:180-184): does this opt track?
    bool opt_tracks()
    {
        opt_n0 = n_opts; opt_s0 = soft_update_counter;
        soft_update_counter += 1;
        if (soft_update_counter != cfg.soft_update_interval) return false;
        soft_update_counter = 0;
        return true;
    }
    // After a synchronisation: the updates whose reduce + Adam launch was skipped (an out-of-range action: every update from the
    // flagged one until the word is cleared) took no optimizer step and no soft update.  The Adam step number goes back to the last
    // applied one, and n_opts and soft_update_counter to what they were before the opt that holds the first skipped update (an opt
    // counts when all its updates were applied; of the last 4096 enqueued updates - older ones keep their counts).
    int32_t settle()
    {
        unsigned long long ap = 0;
        BDR_HIP(hipMemcpy(&ap, applied, sizeof ap, hipMemcpyDeviceToHost));
        if (ap < step) {
            for (const Mark& mk : marks)
                if (mk.step == ap + 1) { n_opts = mk.n_opts; soft_update_counter = mk.soft; break; }
            step = ap;
        }
        marks.clear();
        return BDR_OK;
    }
    int32_t after_sync() override { return settle(); }
    // the deferred report of an out-of-range action (err_report, also from bdr_agent_opt's poll): the stream is idle and the word
    // cleared, so everything enqueued so far has either been applied or skipped
    void on_action_error() override { (void)settle(); }

    const char* kind() const override { return "candle_dqn"; }
    int32_t opt(bdr_replay* r) override
    {
        BDR_REQUIRE(!r->per, "the candle DQN has no prioritized update: the reference panics on a batch that carries importance weights "
                             "(border-candle-agent/src/dqn/base.rs:135-137); use a uniform ring");
        BDR_REQUIRE(r->obs_bytes == (uint64_t)O * 4, "replay rows do not match DQN (candle) obs dim (f32 rows)");
        BDR_REQUIRE(r->act_bytes == 8, "DQN (candle) reads ONE i64 action per row: the ring's action rows must be 8 bytes, not %llu",
                    (unsigned long long)r->act_bytes);
        BDR_REQUIRE(r->device == device, "agent and replay buffer live on different devices");
        BDR_REQUIRE(!r->frame_stack, "DQN (candle) reads f32 observation rows, not a frame-stack store");
        const int Bn = (int)cfg.batch_size;
        BDR_TRY(ensure_batch(Bn));
        const bool track = opt_tracks();
        for (uint64_t u = 0; u < cfg.n_updates_per_opt; ++u) {
            { Bracket br(this, "sample"); BDR_TRY(replay_sample_on_stream(r, Bn, stream)); }
            BDR_TRY(update(Bn, (const float*)r->b_obs, r->b_act, 8, (const float*)r->b_next, r->b_reward, r->b_term, track && u + 1 == cfg.n_updates_per_opt));
        }
        n_opts += 1;
        return BDR_OK;
    }
    std::vector<NamedTensor> meta() const
    {
        std::vector<NamedTensor> mt;
        candle::mlp_meta(net, "", mt);
        return mt;
    }
    // opt_with_record (dqn/base.rs:307-331): the last update's record (Record::merge keeps the later value), param_stats at
    // verbosity >= 2, then ratio_best_act - always - and the reset of both counters
    void record_keys(std::vector<std::string>& keys) override
    {
        keys = {"loss"};
        if (verbose()) {
            keys.insert(keys.end(), {"pred_mean", "reward_mean", "tgt_mean", "tgt_minus_pred_mean"});
            param_stat_keys(meta(), keys);
        }
        keys.push_back("ratio_best_act");
    }
    int32_t record(float* out, int cap, int* n) override
    {
        const int k = verbose() ? 5 : 1;
        std::vector<float> r(k);
        BDR_HIP(hipMemcpyAsync(r.data(), scal, (size_t)k * 4, hipMemcpyDeviceToHost, stream));
        BDR_HIP(hipStreamSynchronize(stream));
        BDR_TRY(settle());
        if (rec_opt) {
            if (verbose()) {
                std::vector<float> ref(net.ref_total);
                BDR_TRY(get_params(0, ref.data(), ref.size()));
                param_stats(meta(), ref.data(), r);
            }
            r.push_back(n_samples_act == 0 ? 0.f : (float)n_samples_best_act / (float)n_samples_act);
            n_samples_act = 0; n_samples_best_act = 0;
        }
        BDR_REQUIRE((int)r.size() <= cap, "the DQN (candle) record needs %d slots", (int)r.size());
        std::copy(r.begin(), r.end(), out);
        *n = (int)r.size();
        return BDR_OK;
    }

    // ---- Policy::sample (dqn/base.rs:202-230) ----
    bool need_q() const { return q_mode || (train && explorer.kind == BDR_EXPLORER_SOFTMAX); }
    // the device results of an acting call of n rows -> h_q (the calls that read the values) or h_idx (the greedy calls)
    int32_t results_to_host(uint64_t n)
    {
        if (need_q()) { h_q.resize(n * A); return rows_to_host(samp, h_q.data(), n * A); }
        h_idx.resize(n);
        return words_to_host(samp_idx, h_idx.data(), n * 2);   // an i64 index is two 32-bit words
    }
    // the forward of n f32 rows (host rows, or device rows inside with_device_rows) on the agent's acting path
    int32_t run_net(uint64_t n, const float* obs)
    {
        BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
        if (act_fused_on()) return act_fused(nullptr, n, obs, BDR_DTYPE_F32, obs_rows_on_device, obs_rows_on_device ? obs_row_stride : (uint64_t)O * 4, nullptr, nullptr);
        BDR_HIP(hipSetDevice(device));
        BDR_TRY(ensure_batch((int)n));
        int32_t st = pack_acting_obs(obs, n, x_o, net.L[0].Kp);
        if (st == BDR_OK) {
            const float* pp[1] = {p}; const float* xs[1] = {x_o}; std::vector<float*>* as[1] = {&a_on};
            st = mlp_forward(net, 1, pp, xs, as, (int)n, "sample_fwd");
        }
        if (st == BDR_OK) {
            CdqnActArgs a{a_on.back(), net.L.back().Np, A, (int)n, samp, samp_idx};
            Bracket br(this, "cdqn_act");
            const hipError_t e = step_launch(stream, false, k_cdqn_act, dim3((unsigned)((n * A + 255) / 256)), dim3(256), a);
            if (e != hipSuccess) st = fail(BDR_ERR_HIP, "k_cdqn_act: %s", hipGetErrorString(e));
        }
        if (st == BDR_OK) st = results_to_host(n);
        if (st == BDR_OK) prof_collect(this);
        slot_cursor = 0;
        return st;
    }
    // the device's error words after an acting call, as bdr_agent_sample reads them
    int32_t acting_errors()
    {
        if (err_fresh) { err_fresh = false; return err_poll(); }
        return err_check();
    }
    static int argmax_host(const float* q, int A)   // dqn_q_argmax's rule
    {
        int best = 0;
        for (int k = 1; k < A; ++k) if (q[k] > q[best]) best = k;
        return best;
    }
    // the explorer on the host, after the forward: the actions of n rows from h_q / h_idx
    int32_t explore(uint64_t n, int64_t* act_out, bdr_sample_info* info)
    {
        double eps = 0.0;
        bool is_random = false;
        if (train) {
            n_samples_act += 1;                                               // dqn/base.rs:205
            if (explorer.kind == BDR_EXPLORER_SOFTMAX) {                      // explorer.rs:31-40
                std::vector<float> pr(A), cum(A);
                for (uint64_t i = 0; i < n; ++i) {
                    SmallRng::softmax_row(&h_q[i * A], A, pr.data());
                    int k = 0;
                    if (!rng.weighted_index(pr.data(), A, cum.data(), &k))
                        return fail(BDR_ERR_INVALID, "Softmax explorer: row %llu of the action values has no valid weights (a NaN or all-zero softmax row): "
                                                     "the reference's WeightedIndex::new(..).unwrap() panics (dqn/explorer.rs:37)", (unsigned long long)i);
                    act_out[i] = k;
                }
            } else {                                                          // explorer.rs:79-133
                Explorer& x = explorer;
                const double d = (x.eps_start - x.eps_final) / (double)x.final_step;
                eps = std::max(x.eps_start - d * (double)x.n_calls, x.eps_final);
                const float r = rng.gen_f32();
                is_random = r < (float)eps;
                x.n_calls += 1;
                bool all_best = true;
                for (uint64_t i = 0; i < n; ++i) {
                    const int64_t act = is_random ? (int64_t)(rng.next_u64() % (uint64_t)A) : h_idx[i];
                    all_best = all_best && act == h_idx[i];
                    act_out[i] = act;
                }
                if (verbose() && all_best) n_samples_best_act += 1;           // action_with_best, dqn/base.rs:209-214
            }
        } else {                                                              // dqn/base.rs:221-227
            if (rng.gen_f32() < 0.01f) {
                is_random = true;
                const int64_t act = rng.gen_range((uint64_t)A);               // ONE action; written to every row
                for (uint64_t i = 0; i < n; ++i) act_out[i] = act;
            } else {
                for (uint64_t i = 0; i < n; ++i) act_out[i] = h_idx[i];
            }
        }
        if (info) {
            info->eps = eps; info->is_random = is_random ? 1 : 0;
            info->n_samples_act = n_samples_act; info->n_samples_best_act = n_samples_best_act;
        }
        return BDR_OK;
    }
    bool sample_i64(uint64_t n, const void* obs, int64_t* act_out, bdr_sample_info* info, int32_t* st) override
    {
        *st = [&]() -> int32_t {
            err_fresh = false;
            BDR_TRY(run_net(n, static_cast<const float*>(obs)));
            BDR_TRY(acting_errors());
            return explore(n, act_out, info);
        }();
        return true;
    }
    bool qvalues_f32(uint64_t n, const void* obs, float* q, int32_t* st) override
    {
        q_mode = true;
        *st = run_net(n, static_cast<const float*>(obs));
        q_mode = false;
        if (*st == BDR_OK) std::copy(h_q.begin(), h_q.begin() + n * A, q);
        return true;
    }
    void explorer_reseed(uint64_t seed) override { rng.seed_from_u64(seed); }
    int32_t sample_raw(const bdr_obs_norm* norm, uint64_t n, const void* rows, int32_t dtype, bool on_device, uint64_t stride, float* act_out,
                       int64_t* idx_out) override
    {
        BDR_REQUIRE(idx_out, "DQN (candle) sample: the actions are i64 indices, written to idx_out");
        err_fresh = false;
        BDR_TRY(DenseAgent::sample_raw(norm, n, rows, dtype, on_device, stride, act_out, idx_out));
        BDR_TRY(acting_errors());
        return explore(n, idx_out, nullptr);
    }
    // ---- DenseAgent's acting hooks (dense_agent.hpp) ----
    const MlpLayout& act_net() const override { return net; }
    const float* act_params() const override { return p; }
    // (the internal calls - run_net - pass no output pointers: the results stay in h_q / h_idx for the explorer)
    int32_t act_check_out(const float*, const int64_t*) const override { return BDR_OK; }
    int32_t act_epilogue(DenseActArgs& a, uint64_t n) override
    {
        BDR_TRY(ensure_batch((int)n));
        a.mode = DA_DQN; a.kind = BDR_ACTIVATION_NONE; a.out = samp; a.idx = samp_idx;
        return BDR_OK;
    }
    int32_t act_results(uint64_t n, float*, int64_t*) override { return results_to_host(n); }
    int32_t act_layers(uint64_t n, const void* rows, bool on_device, uint64_t stride, float*, int64_t*) override
    {
        if (!on_device) return run_net(n, static_cast<const float*>(rows));
        return with_device_rows(rows, stride, [&](const float* r) { return run_net(n, r); });
    }

    // ---- parameter views: 0 qnet, 1 qnet_tgt, 2 exp_avg, 3 exp_avg_sq, 4 grad (the tch Dqn's numbers); also model 0's roles
    // +100 grad, +200 exp_avg, +300 exp_avg_sq (the other dense agents' numbers) ----
    float* slot(int which) const
    {
        switch (which) {
            case 0: return p; case 1: return p_tgt; case 2: case 200: return m; case 3: case 300: return v; case 4: case 100: return g;
            default: return nullptr;
        }
    }
    uint64_t param_count(int which) override { return which == -1 ? (uint64_t)A : slot(which) ? net.ref_total : 0; }
    int32_t get_params(int which, float* out, uint64_t n) override
    {
        float* s = slot(which);
        BDR_REQUIRE(s, "unknown DQN (candle) model %d", which);
        BDR_REQUIRE(n == net.ref_total, "parameter count mismatch (%llu vs %llu)", (unsigned long long)n, (unsigned long long)net.ref_total);
        std::vector<float> in(net.total);
        return arena_to_reference(net, s, in, out);
    }
    int32_t set_params(int which, const float* inp, uint64_t n) override
    {
        float* s = slot(which);
        BDR_REQUIRE(s, "unknown DQN (candle) model %d", which);
        BDR_REQUIRE(n == net.ref_total, "parameter count mismatch");
        std::vector<float> in(net.total, 0.f);
        return arena_from_reference(net, inp, in, s);
    }
    float* arena(int which, size_t* n) override { float* s = slot(which); if (n) *n = s ? net.total : 0; return s; }

    // ---- checkpoints: qnet.pt, qnet_tgt.pt (dqn/base.rs:337-351), VarMaps with mlp.ln{i}.weight / .bias at their root ----
    int32_t save(const char* dir) override
    {
        std::vector<float> w(net.ref_total);
        const char* stems[2] = {"qnet", "qnet_tgt"};
        for (int i = 0; i < 2; ++i) {
            BDR_TRY(get_params(i, w.data(), w.size()));
            BDR_TRY(save_safetensors_named(candle::ckpt_save_path(ckpt_format, dir, stems[i]), meta(), w.data(), w.size()));
        }
        return BDR_OK;
    }
    int32_t load(const char* dir) override
    {
        std::vector<float> w(net.ref_total);
        const char* stems[2] = {"qnet", "qnet_tgt"};
        for (int i = 0; i < 2; ++i) {
            BDR_TRY(load_safetensors_named(candle::ckpt_load_path(ckpt_format, dir, stems[i]), meta(), w.data(), w.size()));
            BDR_TRY(set_params(i, w.data(), w.size()));
        }
        return BDR_OK;
    }
};

namespace {

int32_t cdqn_check(const bdr_candle_dqn_config& c)
{
    BDR_REQUIRE(c.device >= 0, "No device is given for DQN agent");   // dqn/base.rs:245-248
    BDR_REQUIRE(c.obs_dim >= 1 && c.obs_dim <= 4096, "bad obs dim");
    BDR_REQUIRE(c.n_actions >= 1 && c.n_actions <= 4096, "n_actions must be in [1, 4096], got %d", c.n_actions);
    BDR_TRY(check_mlp(c.qnet, "qnet", false));
    BDR_REQUIRE(c.batch_size >= 1 && c.batch_size <= 65536, "bad batch size");
    BDR_REQUIRE(c.soft_update_interval >= 1 && c.n_updates_per_opt >= 1, "intervals must be >= 1");
    BDR_REQUIRE(c.critic_loss == BDR_LOSS_MSE || c.critic_loss == BDR_LOSS_SMOOTH_L1, "unknown critic loss %d", c.critic_loss);
    BDR_TRY(check_opt(c.opt, "qnet"));
    BDR_REQUIRE(c.explorer.kind == BDR_EXPLORER_SOFTMAX || c.explorer.kind == BDR_EXPLORER_EPS_GREEDY, "unknown explorer kind");
    BDR_REQUIRE(c.explorer.kind != BDR_EXPLORER_EPS_GREEDY || c.explorer.final_step > 0, "final_step must be positive");
    BDR_REQUIRE(c.ckpt_format == BDR_CKPT_TCH || c.ckpt_format == BDR_CKPT_SAFETENSORS, "unknown checkpoint format");
    return BDR_OK;
}

}  // namespace

extern "C" {

void bdr_candle_dqn_config_default(bdr_candle_dqn_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof *c);
    // dqn/config.rs:75-102
    c->soft_update_interval = 1; c->n_updates_per_opt = 1; c->batch_size = 1;
    c->discount_factor = 0.99; c->tau = 0.005; c->train = 0;
    bdr_explorer_config_default(&c->explorer, BDR_EXPLORER_SOFTMAX);
    c->explorer.seed = 42;   // dqn/base.rs:274
    c->has_clip_reward = 0; c->double_dqn = 0; c->has_clip_td_err = 0; c->device = -1;
    c->critic_loss = BDR_LOSS_MSE; c->record_verbose_level = 0;
    // DqnModelConfig (dqn/model.rs:32-39): opt_config = OptimizerConfig::default() = AdamW with candle's ParamsAdamW defaults (opt.rs:100-111)
    c->qnet.activation_out = BDR_ACTIVATION_NONE;
    c->lr = 1e-3;
    c->opt.opt_kind = BDR_OPT_ADAMW; c->opt.beta1 = 0.9; c->opt.beta2 = 0.999; c->opt.weight_decay = 0.01; c->opt.eps = 1e-8;
    c->ckpt_format = BDR_CKPT_TCH;
}

int32_t bdr_candle_dqn_create(const bdr_candle_dqn_config* cfg, bdr_agent** out)
{
    BDR_REQUIRE(cfg && out, "null argument");
    const bdr_candle_dqn_config& c = *cfg;
    BDR_TRY(cdqn_check(c));
    BDR_TRY(ensure_device(c.device));
    CandleDqn* a = new CandleDqn();
    a->cfg = c; a->device = c.device; a->train = c.train != 0; a->ckpt_format = c.ckpt_format;
    a->O = c.obs_dim; a->A = c.n_actions;
    a->net = make_mlp(c.obs_dim, c.qnet.units, c.qnet.n_units, c.n_actions, c.qnet.activation_out == BDR_ACTIVATION_RELU);
    Explorer& x = a->explorer;
    x.kind = c.explorer.kind; x.eps_start = c.explorer.eps_start; x.eps_final = c.explorer.eps_final; x.final_step = c.explorer.final_step;
    x.n_calls = c.explorer.n_calls;
    a->rng.seed_from_u64(c.explorer.seed);
    const MlpLayout& net = a->net;
    const int32_t st = [&]() -> int32_t {
        BDR_HIP(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
        BDR_TRY(a->err_init());
        for (auto q : {&a->p, &a->p_tgt, &a->g, &a->m, &a->v}) BDR_TRY(a->alloc(q, net.total, CandleDqn::AGENT));
        BDR_TRY(a->alloc(&a->scal, 8, CandleDqn::AGENT));
        BDR_TRY(a->alloc(&a->applied, 1, CandleDqn::AGENT));
        std::vector<float> ref(net.ref_total, 0.f);
        mlp_init_reference(net, c.seed * 7 + 1, ref.data());
        BDR_TRY(a->set_params(0, ref.data(), ref.size()));
        BDR_TRY(a->set_params(1, ref.data(), ref.size()));   // track(qnet_tgt, qnet, 1.0) (dqn/base.rs:251)
        return a->ensure_batch((int)c.batch_size);
    }();
    if (st != BDR_OK) { delete a; return st; }
    *out = a;
    return BDR_OK;
}

int32_t bdr_candle_dqn_update_on_batch(bdr_agent* base, uint64_t n, const float* obs, const int64_t* act, const float* next_obs, const float* reward,
                                       const int8_t* term, const int8_t* /*is_truncated: read by nothing, dqn/base.rs:62*/, bdr_dqn_record* rec)
{
    BDR_REQUIRE(base && obs && act && next_obs && reward && term, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "candle_dqn"), "not a DQN (candle) agent");
    CandleDqn* a = static_cast<CandleDqn*>(base);
    BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
    BDR_HIP(hipSetDevice(a->device));
    BDR_TRY(a->ensure_batch((int)n));
    if (n > a->u_cap) {
        BDR_HIP(hipStreamSynchronize(a->stream));
        a->release(CandleDqn::STAGING);
        a->u_cap = 0;
        BDR_TRY(a->alloc(&a->u_obs, n * a->O, CandleDqn::STAGING, false)); BDR_TRY(a->alloc(&a->u_next, n * a->O, CandleDqn::STAGING, false));
        BDR_TRY(a->alloc(&a->u_act, n, CandleDqn::STAGING, false)); BDR_TRY(a->alloc(&a->u_rew, n, CandleDqn::STAGING, false));
        BDR_TRY(a->alloc(&a->u_term, round_up(n, 16), CandleDqn::STAGING, false));
        a->u_cap = n;
    }
    BDR_HIP(hipMemcpyAsync(a->u_obs, obs, n * a->O * 4, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_next, next_obs, n * a->O * 4, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_act, act, n * 8, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_rew, reward, n * 4, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_term, term, n, hipMemcpyHostToDevice, a->stream));
    const bool track = a->opt_tracks();
    BDR_TRY(a->update((int)n, a->u_obs, reinterpret_cast<const uint8_t*>(a->u_act), 8, a->u_next, a->u_rew, a->u_term, track));
    a->n_opts += 1;
    prof_collect(a);
    float r5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    BDR_HIP(hipMemcpyAsync(r5, a->scal, sizeof r5, hipMemcpyDeviceToHost, a->stream));
    BDR_HIP(hipStreamSynchronize(a->stream));
    BDR_TRY(a->settle());
    if (rec) {
        rec->loss = r5[0]; rec->has_verbose = a->verbose() ? 1 : 0;
        if (a->verbose()) { rec->pred_mean = r5[1]; rec->reward_mean = r5[2]; rec->tgt_mean = r5[3]; rec->tgt_minus_pred_mean = r5[4]; }
    }
    return a->err_check();
}

// Parity probes of the LAST update (see include/border_amd.h)
int32_t bdr_candle_dqn_probe(bdr_agent* base, int32_t what, float* out, uint64_t n)
{
    BDR_REQUIRE(base && out, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "candle_dqn"), "not a DQN (candle) agent");
    CandleDqn* a = static_cast<CandleDqn*>(base);
    BDR_HIP(hipSetDevice(a->device));
    BDR_REQUIRE(a->last_B > 0, "no update has run yet");
    BDR_REQUIRE(what >= 0 && what <= 4, "unknown DQN (candle) probe %d", what);
    BDR_REQUIRE(n == (uint64_t)a->last_B, "this probe holds batch values");
    const float* src[5] = {a->pr_pred, a->pr_qn, a->pr_y, a->pr_tgt, a->pr_dpred};
    BDR_HIP(hipStreamSynchronize(a->stream));
    BDR_HIP(hipMemcpy(out, src[what], n * 4, hipMemcpyDeviceToHost));
    return BDR_OK;
}

}  // extern "C"
