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
// The AtariCnn Q-network (atari_cnn/base.rs) is the second form, CandleDqnCnn below: the shared conv trunk (conv_trunk.hpp) in front
// of the same head and TD step, and k_cdqn_conv_reduce_adam, the candle optimizer step over the conv gradients' partial sums.
#include <algorithm>
#include <cstdlib>
#include <deque>

#include "candle_actor.hpp"
#include "conv_trunk.hpp"
#include "candle_dqn_group_plan.hpp"

using namespace bdr;

namespace {

// obs, next_obs [B][O] -> the zero-padded first-layer inputs x_o, x_no [B][Kp] in one launch (the padding columns were zeroed when
// the buffers were allocated and are never written).  Bounds: t < B O; row b < B, column c < O <= Kp.
// (the body over its operands: the kernel's arguments, or a member's entry of a group's device array - candle_dqn_group.hpp)
__device__ __forceinline__ void cdqn_pack_body(const float* __restrict__ obs, const float* __restrict__ next_obs, int O, int Kp, int B,
                                               float* __restrict__ x_o, float* __restrict__ x_no)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * O) return;
    const size_t d = (size_t)(t / O) * Kp + t % O;
    x_o[d] = obs[t];
    x_no[d] = next_obs[t];
}
__global__ __launch_bounds__(256) void k_cdqn_pack(const float* __restrict__ obs, const float* __restrict__ next_obs, int O, int Kp, int B,
                                                   float* __restrict__ x_o, float* __restrict__ x_no)
{
    cdqn_pack_body(obs, next_obs, O, Kp, B, x_o, x_no);
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
template <class Args>
__device__ __forceinline__ long long cdqn_action(const Args& p, int b, bool* bad)
{
    long long a = *reinterpret_cast<const long long*>(p.act + (size_t)b * p.act_bytes);
    *bad = a < 0 || a >= p.A;
    if (*bad) a = a < 0 ? 0 : p.A - 1;
    return a;
}
// (the body over its argument struct: the kernel argument, or a member's entry of a group's device array read in place through the
// constant address space - k_cdqn_td_group, candle_dqn_group.hpp; red: the workgroup's float[32])
template <class Args>
__device__ __forceinline__ void cdqn_td_body(const Args& p, float* red)
{
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
__global__ __launch_bounds__(1024) void k_cdqn_td(CdqnTdArgs p)
{
    __shared__ float red[32];
    cdqn_td_body(p, red);
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

// ---- k_cdqn_conv_reduce_adam ------------------------------------------------------------------------------------------------------
// The optimizer step of the AtariCnn form's conv parameters.  The conv weight-gradient kernels (DwC3, DwC2, conv1_dw_bf16) leave
// row-chunk partials [chunks][K N + N] (weights, then bias) per layer.  A workgroup owns 32 float4 of the conv arena W1 b1 W2 b2 W3 b3 -
// the segments follow one another without slack, each a multiple of four floats - and eight threads share a float4 i
// (cnn_layers.hpp reduce_partials_8x32, the sum the tch DQN's k_reduce_adam runs over floats):
//   thread group q = 0 ... 7 sums the float4 of the chunks c = q, q + 8, ... in ascending order; the eight sums meet in LDS and
//   group 0 adds them as ((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7: ONE order, whatever the grid (conv1 leaves up to 256
//   chunks: one thread per float4 walked them in 82 us at B = 256); it scales conv1's WEIGHT elements by 1/255 (the kernel multiplied
//   raw u8 operands; the bias gradient is the plain column sum), stores the gradient arena,
//   applies adam_element (candle AdamW / candle-optimisers Adam through AdamScalars) and, on the opts that track, track_element -
//   exactly what k_dense_reduce_adam applies to the head's parameters.
// It reads the same poison word (err[ERR_ACTION], raised by k_cdqn_td earlier in the same update) and writes the same `applied`
// word as the head's launch: the word does not change between the two launches of an update (only the host clears it, with the
// stream idle), so either every parameter of an update steps or none does, and settle() holds for the whole set.
// Bounds.  i = 32 blockIdx.x + (threadIdx.x & 31) < n4 = conv floats / 4 for every access but the LDS store (red[8][32], indexed by
// the thread's group and slot); segment k = the last one with off4 <= i, so j = i - off4 < seg.n4 and the reads
// part[c * stride + 4 j .. + 3], c < chunks, stay below chunks * stride (stride = 4 seg.n4 = the segment's floats).  p, g, m, v, tgt
// are arenas of at least n4 float4.
struct CdqnConvSeg { const float* part; size_t stride; int chunks; unsigned off4, n4, nw4; float wscale; };   // float4s [off4, off4 + n4); the first nw4 scaled
struct CdqnConvAdamArgs {
    CdqnConvSeg seg[3];
    float *p, *g, *m, *v, *tgt;
    AdamScalars s; unsigned n4; float tau, omt; int track;
    const unsigned* poison; unsigned long long* applied; unsigned long long step;
};
__global__ __launch_bounds__(256) void k_cdqn_conv_reduce_adam(CdqnConvAdamArgs a)
{
#pragma clang fp contract(off)
    __shared__ f32x4 red[8][32];
    if (*a.poison) return;   // (the whole grid reads the same word: no thread of a workgroup is left at the barrier)
    const unsigned i = blockIdx.x * 32 + (threadIdx.x & 31);
    const int k = (i >= a.seg[1].off4 ? 1 : 0) + (i >= a.seg[2].off4 ? 1 : 0);
    const CdqnConvSeg sg = a.seg[k];
    const unsigned j = i - sg.off4;
    reduce_partials_8x32(red, sg, j, i < a.n4, [&](f32x4 gg) {
#pragma clang fp contract(off)
        if (i == 0) *a.applied = a.step;
        if (j < sg.nw4) gg *= sg.wscale;
        reinterpret_cast<f32x4*>(a.g)[i] = gg;
        f32x4 pp = reinterpret_cast<f32x4*>(a.p)[i], mm = reinterpret_cast<f32x4*>(a.m)[i], vv = reinterpret_cast<f32x4*>(a.v)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pe = pp[e], me = mm[e], ve = vv[e];
            adam_element(pe, gg[e], me, ve, a.s);
            pp[e] = pe; mm[e] = me; vv[e] = ve;
        }
        reinterpret_cast<f32x4*>(a.p)[i] = pp;
        reinterpret_cast<f32x4*>(a.m)[i] = mm;
        reinterpret_cast<f32x4*>(a.v)[i] = vv;
        if (a.track) {
            f32x4 d = reinterpret_cast<f32x4*>(a.tgt)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = track_element(pp[e], d[e], a.tau, a.omt);
            reinterpret_cast<f32x4*>(a.tgt)[i] = d;
        }
    });
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
    int B = 0; uint64_t batch_gen = 0;   // batch_gen: bumped whenever the batch buffers are re-allocated (candle_dqn_group.hpp keys its static arguments on it)
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
    // The AtariCnn form (CandleDqnCnn below) keeps a conv trunk in front of `net`: it brings the trunk's batch buffers in place of
    // the packed f32 inputs, its own forward of an acting call, and the sizes and names of the whole parameter set
    virtual bool cnn_form() const { return false; }
    virtual int32_t alloc_inputs(int Bn)
    {
        BDR_TRY(alloc(&x_o, (size_t)Bn * net.L[0].Kp, BATCH));
        return alloc(&x_no, (size_t)Bn * net.L[0].Kp, BATCH);
    }
    virtual uint64_t ref_count() const { return net.ref_total; }
    virtual size_t arena_floats() const { return net.total; }

    int32_t ensure_batch(int Bn)
    {
        if (Bn <= B) return BDR_OK;
        BDR_HIP(hipStreamSynchronize(stream));
        release(BATCH);
        B = 0;
        BDR_TRY(alloc_inputs(Bn));
        for (auto* vec : {&a_on, &a_tg, &a_onn, &dy}) BDR_TRY(layer_bufs(net, Bn, *vec));
        for (auto q : {&pr_pred, &pr_qn, &pr_y, &pr_tgt, &pr_dpred, &lrow}) BDR_TRY(alloc(q, Bn, BATCH));
        BDR_TRY(alloc(&part, plan(net, Bn, off), BATCH));
        BDR_TRY(alloc(&samp, (size_t)Bn * A, BATCH));
        BDR_TRY(alloc(&samp_idx, Bn, BATCH));
        B = Bn; batch_gen += 1;
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
    virtual std::vector<NamedTensor> meta() const
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
                std::vector<float> ref(ref_count());
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
    virtual int32_t run_net(uint64_t n, const float* obs)
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
    bool param_view(int which, ParamView* pv) override
    {
        if (!slot(which)) return false;
        *pv = net_view(slot(which));
        return true;
    }
    virtual ParamView net_view(float* arena) { return mlp_view(net, arena); }
    int n_actions() const override { return A; }
    // ---- checkpoints: qnet.pt, qnet_tgt.pt (dqn/base.rs:337-351), VarMaps with the variables of meta() at their root ----
    void checkpoint_files(std::vector<CheckpointFile>& files) override { files = {{"qnet", meta(), {0}, {0}}, {"qnet_tgt", meta(), {1}, {1}}}; }
};

// ================================================================================================
// The AtariCnn form (border-candle-agent/src/atari_cnn/base.rs:31-45): conv1 8x8/4, conv2 4x4/2, conv3 3x3/1 with ReLU after each -
// the shared layer policies of cnn_layers.hpp, driven by conv_trunk.hpp as IQN's psi is - then `net` = [3136 -> 512 -> A] on DenseAgent's
// kernels.  Every arena is  W1 b1 W2 b2 W3 b3 (conv_layout.hpp's layouts) | net's arena;  conv3's output [B][7][7][64] is net's first
// input as it stands, and l1.weight's 3136 columns, (c, h, w) in the reference, are permuted once in to_internal / to_reference.
// Arithmetic: conv1 on the bf16 MFMA with exact u8 operands and the 1/255 in its epilogue, everything else f32 x f32 on the FP32
// MFMA (BDR_ARITH_F32_EXACT of the tch agent).  One queue, eager launches.  One update is
//   3 trunk forwards (conv1, conv2, conv3: the passes (p, obs), (p_tgt, next_obs) and - double_dqn - (p, next_obs) share a launch)
//   2 head forwards, k_cdqn_td, 2 head input gradients (l2, then d(features) under conv3's ReLU mask), the grouped dW of l1 and l2,
//   the head's reduce + Adam, conv3 dW, conv3 dX, conv2 dW, conv2 dX, conv1 dW, k_cdqn_conv_reduce_adam
// = 16 launches plus the ring's gather.  The head steps before the trunk's backward runs; nothing behind it reads l1 or l2.
struct CandleDqnCnn : CandleDqn {
    bdr_candle_dqn_cnn_config ccfg;
    Arena conv;                      // offsets of W1 ... b3 (w4 = the conv floats = where net's arena begins)
    float *a1[3] = {}, *a2[3] = {}, *a3[3] = {};    // trunk activations of the three passes
    float *dy3 = nullptr, *dy2 = nullptr, *dy1 = nullptr, *part_conv = nullptr;
    uint8_t *u_obs8 = nullptr, *u_next8 = nullptr; uint64_t u_cap8 = 0;

    bool cnn_form() const override { return true; }
    size_t conv_floats() const { return conv.w4; }
    size_t row_bytes() const { return (size_t)7056 * conv.ns; }
    uint64_t ref_count() const override { return (uint64_t)conv_floats() + net.ref_total; }
    size_t arena_floats() const override { return conv_floats() + net.total; }
    float* head(float* arena_base) const { return arena_base + conv_floats(); }

    int32_t alloc_inputs(int Bn) override
    {
        for (int z = 0; z < 3; ++z) {
            BDR_TRY(alloc(&a1[z], Bn * CONV_A1_ROW, BATCH)); BDR_TRY(alloc(&a2[z], Bn * CONV_A2_ROW, BATCH)); BDR_TRY(alloc(&a3[z], Bn * CONV_A3_ROW, BATCH));
        }
        BDR_TRY(alloc(&dy3, Bn * CONV_A3_ROW, BATCH)); BDR_TRY(alloc(&dy2, Bn * CONV_A2_ROW, BATCH)); BDR_TRY(alloc(&dy1, Bn * CONV_A1_ROW, BATCH));
        return alloc(&part_conv, conv_dw_plan(conv, Bn).total, BATCH);
    }
    // the trunk of nz (parameters, u8 rows) pairs into a1 / a2 / a3 [0, nz): one launch per layer
    int32_t trunk_forward(int nz, const float* const* pp, const uint8_t* const* rows, int Bn, const char* name)
    {
        BDR_TRY(trunk_conv1(this, conv, nz, pp, rows, a1, Bn, name));
        return trunk_conv23(this, conv, nz, pp, a1, a2, a3, Bn, name, name);
    }
    int32_t update_cnn(int Bn, const uint8_t* obs, const uint8_t* act, int act_bytes, const uint8_t* next_obs, const float* reward, const int8_t* term, bool track)
    {
        BDR_TRY(ensure_batch(Bn));
        const int L = (int)net.L.size(), nz = cfg.double_dqn ? 3 : 2;
        const DenseLayer& last = net.L[L - 1];
        {
            const float* pp[3] = {p, p_tgt, p}; const uint8_t* rows[3] = {obs, next_obs, next_obs};
            BDR_TRY(trunk_forward(nz, pp, rows, Bn, "fwd_conv"));
            const float* hp[3] = {head(p), head(p_tgt), head(p)}; const float* xs[3] = {a3[0], a3[1], a3[2]}; std::vector<float*>* as[3] = {&a_on, &a_tg, &a_onn};
            BDR_TRY(mlp_forward(net, nz, hp, xs, as, Bn, "fwd"));
        }
        {
            CdqnTdArgs t{};
            t.q_on = a_on[L - 1]; t.q_tg = a_tg[L - 1]; t.q_on_next = cfg.double_dqn ? a_onn[L - 1] : nullptr;
            t.Np = last.Np; t.A = A; t.B = Bn; t.act = act; t.act_bytes = act_bytes; t.reward = reward; t.term = term;
            t.gamma = (float)cfg.discount_factor; t.loss_kind = cfg.critic_loss; t.relu_out = 0; t.verbose = verbose() ? 1 : 0;
            t.dy = dy[L - 1]; t.pred = pr_pred; t.q_next = pr_qn; t.y = pr_y; t.tgt = pr_tgt; t.dpred = pr_dpred; t.lrow = lrow;
            t.scal = scal; t.err = dev_err;
            Bracket br(this, "cdqn_td");
            BDR_HIP(step_launch(stream, false, k_cdqn_td, dim3(1), dim3(1024), t));
        }
        step += 1;
        marks.push_back(Mark{step, opt_n0, opt_s0});
        if (marks.size() > 4096) marks.pop_front();
        const AdamScalars sc = opt_scalars(cfg.opt, cfg.lr, step);
        {   // the head: l2's and l1's input gradients (the second one is d(features) under conv3's ReLU mask), dW, reduce + Adam
            std::vector<float*>* acts[1] = {&a_on}; std::vector<float*>* dys[1] = {&dy};
            float *hp = head(p), *hg = head(g), *hm = head(m), *hv = head(v), *ht[1] = {head(p_tgt)};
            float* dx0[1] = {dy3}; const float* mask0[1] = {a3[0]};
            BDR_TRY(mlp_backward_step(net, 1, &hp, &hg, &hm, &hv, track ? ht : nullptr, a3[0], acts, dys, part, 0, off, &sc, Bn, {"dx", "dw", "reduce_adam"}, net.total,
                                      cfg.tau, L - 1, nullptr, dev_err + ERR_ACTION, applied, step, dx0, mask0));
        }
        CdqnConvAdamArgs ra{};
        int k = 3;   // the hook runs for conv3, conv2, conv1; the segments are in arena order
        BDR_TRY(trunk_backward(this, conv, p, obs, a1[0], a2[0], dy3, dy2, dy1, part_conv, Bn, B, "", [&](const ConvDwLayer& l, int chunks, const float* lp) {
            ra.seg[--k] = CdqnConvSeg{lp, l.stride, chunks, (unsigned)(l.w / 4), (unsigned)(l.n / 4), (unsigned)(l.n_weights / 4), l.wscale};
            return (int32_t)BDR_OK;
        }));
        {
            ra.p = p; ra.g = g; ra.m = m; ra.v = v; ra.tgt = p_tgt; ra.s = sc; ra.n4 = (unsigned)(conv_floats() / 4);
            ra.track = track ? 1 : 0; ra.tau = (float)cfg.tau; ra.omt = (float)(1.0 - cfg.tau);
            ra.poison = dev_err + ERR_ACTION; ra.applied = applied; ra.step = step;
            Bracket br(this, "conv_reduce_adam");
            BDR_HIP(step_launch(stream, true, k_cdqn_conv_reduce_adam, dim3((ra.n4 + 31) / 32), dim3(256), ra));
        }
        last_B = Bn;
        return BDR_OK;
    }
    int32_t opt(bdr_replay* r) override
    {
        BDR_REQUIRE(!r->per, "the candle DQN has no prioritized update: the reference panics on a batch that carries importance weights "
                             "(border-candle-agent/src/dqn/base.rs:135-137); use a uniform ring");
        BDR_REQUIRE(r->obs_bytes != (uint64_t)row_bytes() * 4, "DQN (candle, AtariCnn) reads u8 observation rows of 84 x 84 x n_stack bytes, not an f32 ring");
        BDR_REQUIRE(r->obs_bytes == (uint64_t)row_bytes(), "replay rows of %llu bytes do not match DQN (candle, AtariCnn) u8 rows of 84 x 84 x %d = %llu bytes",
                    (unsigned long long)r->obs_bytes, conv.ns, (unsigned long long)row_bytes());
        BDR_REQUIRE(r->act_bytes == 8, "DQN (candle) reads ONE i64 action per row: the ring's action rows must be 8 bytes, not %llu",
                    (unsigned long long)r->act_bytes);
        BDR_REQUIRE(r->device == device, "agent and replay buffer live on different devices");
        const int Bn = (int)cfg.batch_size;
        BDR_TRY(ensure_batch(Bn));
        const bool track = opt_tracks();
        for (uint64_t u = 0; u < cfg.n_updates_per_opt; ++u) {
            { Bracket br(this, "sample"); BDR_TRY(replay_sample_on_stream(r, Bn, stream)); }
            BDR_TRY(update_cnn(Bn, r->b_obs, r->b_act, 8, r->b_next, r->b_reward, r->b_term, track && u + 1 == cfg.n_updates_per_opt));
        }
        n_opts += 1;
        return BDR_OK;
    }
    std::vector<NamedTensor> meta() const override
    {
        return {{"c1.weight", {32, (uint64_t)conv.ns, 8, 8}}, {"c1.bias", {32}}, {"c2.weight", {64, 32, 4, 4}}, {"c2.bias", {64}},
                {"c3.weight", {64, 64, 3, 3}}, {"c3.bias", {64}}, {"l1.weight", {512, 3136}}, {"l1.bias", {512}},
                {"l2.weight", {(uint64_t)A, 512}}, {"l2.bias", {(uint64_t)A}}};
    }
    // Policy::sample's forward: u8 rows (host rows, or device rows inside a DeviceRowsScope) through the batch forward of the update
    int32_t run_net(uint64_t n, const float* obs) override
    {
        BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
        BDR_HIP(hipSetDevice(device));
        BDR_TRY(ensure_batch((int)n));
        const uint8_t* d = nullptr;
        int32_t st = acting_rows(obs, row_bytes(), n, &d);
        if (st == BDR_OK) { const float* pp[1] = {p}; const uint8_t* rows[1] = {d}; st = trunk_forward(1, pp, rows, (int)n, "sample_conv"); }
        if (st == BDR_OK) {
            const float* hp[1] = {head(p)}; const float* xs[1] = {a3[0]}; std::vector<float*>* as[1] = {&a_on};
            st = mlp_forward(net, 1, hp, xs, as, (int)n, "sample_fwd");
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
    int32_t set_act_path(int32_t path) override
    {
        BDR_REQUIRE(path == BDR_ACT_PATH_DEFAULT || path == BDR_ACT_PATH_LAYERS || path == BDR_ACT_PATH_FUSED, "unknown act path %d", path);
        BDR_REQUIRE(path != BDR_ACT_PATH_FUSED, "the fused acting kernel runs Mlp networks on f32 rows: the AtariCnn Q-network of this DQN (candle) agent acts "
                                                "through its layer launches (BDR_ACT_PATH_LAYERS)");
        return BDR_OK;
    }
    int32_t sample_raw(const bdr_obs_norm*, uint64_t, const void*, int32_t, bool, uint64_t, float*, int64_t*) override
    {
        return fail(BDR_ERR_INVALID, "bdr_agent_sample_raw takes f32 / f64 rows: the AtariCnn Q-network of this DQN (candle) agent reads u8 frame stacks "
                                     "(bdr_agent_sample, bdr_agent_sample_device)");
    }

    // ---- reference <-> internal layouts: the conv layers by conv_layout.hpp, l1's input columns (c, h, w) -> (h, w, c) ----
    void to_internal(const float* ref, float* in) const
    {
        std::fill(in, in + arena_floats(), 0.f);
        const float* q = ref + conv_to_internal(conv, ref, in);
        float* h = in + conv_floats();
        const DenseLayer &l1 = net.L[0], &l2 = net.L[1];
        for (int o = 0; o < 512; ++o) for (int j = 0; j < 3136; ++j) h[l1.w + (size_t)((j % 49) * 64 + j / 49) * l1.Np + o] = q[(size_t)o * 3136 + j];
        q += (size_t)512 * 3136; std::copy(q, q + 512, h + l1.b); q += 512;
        for (int o = 0; o < A; ++o) for (int k = 0; k < 512; ++k) h[l2.w + (size_t)k * l2.Np + o] = q[(size_t)o * 512 + k];
        q += (size_t)A * 512; std::copy(q, q + A, h + l2.b);
    }
    void to_reference(const float* in, float* ref) const
    {
        float* q = ref + conv_to_reference(conv, in, ref);
        const float* h = in + conv_floats();
        const DenseLayer &l1 = net.L[0], &l2 = net.L[1];
        for (int o = 0; o < 512; ++o) for (int j = 0; j < 3136; ++j) q[(size_t)o * 3136 + j] = h[l1.w + (size_t)((j % 49) * 64 + j / 49) * l1.Np + o];
        q += (size_t)512 * 3136; std::copy(h + l1.b, h + l1.b + 512, q); q += 512;
        for (int o = 0; o < A; ++o) for (int k = 0; k < 512; ++k) q[(size_t)o * 512 + k] = h[l2.w + (size_t)k * l2.Np + o];
        q += (size_t)A * 512; std::copy(h + l2.b, h + l2.b + A, q);
    }
    ParamView net_view(float* arena) override
    {
        return {arena, arena_floats(), ref_count(), [this](const float* in, float* ref) { to_reference(in, ref); }, [this](const float* ref, float* in) { to_internal(ref, in); }};
    }
};

namespace {

int32_t cdqn_check(const bdr_candle_dqn_config& c)
{
    BDR_REQUIRE(c.device >= 0, "No device is given for DQN agent");   // dqn/base.rs:245-248
    BDR_REQUIRE(c.obs_dim >= 1 && c.obs_dim <= 4096, "bad obs dim");
    BDR_REQUIRE(c.n_actions >= 1 && c.n_actions <= CQ_MAX_ACTIONS, "n_actions must be in [1, %d], got %d", CQ_MAX_ACTIONS, c.n_actions);
    BDR_TRY(check_mlp(c.qnet, "qnet", false));
    BDR_REQUIRE(c.batch_size >= 1 && c.batch_size <= (uint64_t)CQ_MAX_BATCH, "bad batch size");   // (candle_dqn_group_plan.hpp: the limits the TD launch indexes)
    BDR_REQUIRE(c.soft_update_interval >= 1 && c.n_updates_per_opt >= 1, "intervals must be >= 1");
    BDR_REQUIRE(c.critic_loss == BDR_LOSS_MSE || c.critic_loss == BDR_LOSS_SMOOTH_L1, "unknown critic loss %d", c.critic_loss);
    BDR_TRY(check_opt(c.opt, "qnet"));
    BDR_REQUIRE(c.explorer.kind == BDR_EXPLORER_SOFTMAX || c.explorer.kind == BDR_EXPLORER_EPS_GREEDY, "unknown explorer kind");
    BDR_REQUIRE(c.explorer.kind != BDR_EXPLORER_EPS_GREEDY || c.explorer.final_step > 0, "final_step must be positive");
    BDR_REQUIRE(c.ckpt_format == BDR_CKPT_TCH || c.ckpt_format == BDR_CKPT_SAFETENSORS, "unknown checkpoint format");
    return BDR_OK;
}

// the AtariCnn form's config as the shared one (the Mlp fields stay zero), after the checks of its own fields
int32_t cdqn_cnn_check(const bdr_candle_dqn_cnn_config& c, bdr_candle_dqn_config* out)
{
    BDR_REQUIRE(c.skip_linear == 0, "AtariCnnConfig::skip_linear = true leaves the 3136 features of conv3 as the output: Dqn needs out_dim action values (l1, l2)");
    BDR_REQUIRE(c.arithmetic == BDR_ARITH_F32_EXACT, "DQN (candle, AtariCnn) computes exact f32 products in conv2 / conv3 (BDR_ARITH_F32_EXACT): the split-operand "
                                                     "forward (BDR_ARITH_BF16X3_6) is the tch agent's (bdr_dqn_config)");
    BDR_REQUIRE(c.n_stack >= 1 && c.n_stack <= bdr::C1_MAX_STACK, "AtariCnnConfig::n_stack must be in [1, %d] (conv1's kernels are instantiated per depth), got %d",
                bdr::C1_MAX_STACK, c.n_stack);
    bdr_candle_dqn_config d;
    memset(&d, 0, sizeof d);
    d.obs_dim = 1; d.n_actions = c.out_dim; d.qnet.n_units = 1; d.qnet.units[0] = 512; d.qnet.activation_out = BDR_ACTIVATION_NONE;
    d.opt = c.opt; d.lr = c.lr; d.soft_update_interval = c.soft_update_interval; d.n_updates_per_opt = c.n_updates_per_opt; d.batch_size = c.batch_size;
    d.discount_factor = c.discount_factor; d.tau = c.tau; d.train = c.train; d.double_dqn = c.double_dqn; d.explorer = c.explorer;
    d.has_clip_reward = c.has_clip_reward; d.has_clip_td_err = c.has_clip_td_err; d.clip_reward = c.clip_reward;
    d.clip_td_err_min = c.clip_td_err_min; d.clip_td_err_max = c.clip_td_err_max; d.critic_loss = c.critic_loss;
    d.record_verbose_level = c.record_verbose_level; d.device = c.device; d.ckpt_format = c.ckpt_format; d.seed = c.seed;
    BDR_TRY(check_opt(c.opt, "qnet"));   // (amsgrad) before the device is looked at, like the other refusals here
    BDR_REQUIRE(c.batch_size >= 1 && c.batch_size <= 65536, "bad batch size");
    BDR_REQUIRE(c.device >= 0, "No device is given for DQN agent");
    BDR_TRY(cdqn_check(d));
    *out = d;
    return BDR_OK;
}

}  // namespace

#include "candle_dqn_group.hpp"   // the launch grouping of Mlp-form agents: needs CandleDqn and the bodies above

extern "C" {

void bdr_candle_dqn_cnn_config_default(bdr_candle_dqn_cnn_config* c)
{
    if (!c) return;
    bdr_candle_dqn_config d;
    bdr_candle_dqn_config_default(&d);
    memset(c, 0, sizeof *c);
    c->n_stack = 4; c->out_dim = 0; c->skip_linear = 0; c->arithmetic = BDR_ARITH_F32_EXACT;   // atari_cnn/config.rs; the arithmetic is this library's
    c->opt = d.opt; c->lr = d.lr; c->soft_update_interval = d.soft_update_interval; c->n_updates_per_opt = d.n_updates_per_opt; c->batch_size = d.batch_size;
    c->discount_factor = d.discount_factor; c->tau = d.tau; c->train = d.train; c->double_dqn = d.double_dqn; c->explorer = d.explorer;
    c->critic_loss = d.critic_loss; c->record_verbose_level = d.record_verbose_level; c->device = d.device; c->ckpt_format = d.ckpt_format;
}

int32_t bdr_candle_dqn_cnn_create(const bdr_candle_dqn_cnn_config* cfg, bdr_agent** out)
{
    BDR_REQUIRE(cfg && out, "null argument");
    bdr_candle_dqn_config c;
    BDR_TRY(cdqn_cnn_check(*cfg, &c));
    BDR_TRY(ensure_device(c.device));
    CandleDqnCnn* a = new CandleDqnCnn();
    a->ccfg = *cfg; a->cfg = c; a->device = c.device; a->train = c.train != 0; a->ckpt_format = c.ckpt_format;
    a->O = 0; a->A = c.n_actions;
    a->conv = make_arena(1, cfg->n_stack);
    const int units[1] = {512};
    a->net = make_mlp(3136, units, 1, c.n_actions, false);
    Explorer& x = a->explorer;
    x.kind = c.explorer.kind; x.eps_start = c.explorer.eps_start; x.eps_final = c.explorer.eps_final; x.final_step = c.explorer.final_step;
    x.n_calls = c.explorer.n_calls;
    a->rng.seed_from_u64(c.explorer.seed);
    const int32_t st = [&]() -> int32_t {
        BDR_HIP(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
        BDR_TRY(a->err_init());
        for (auto q : {&a->p, &a->p_tgt, &a->g, &a->m, &a->v}) BDR_TRY(a->alloc(q, a->arena_floats(), CandleDqn::AGENT));
        BDR_TRY(a->alloc(&a->scal, 8, CandleDqn::AGENT));
        BDR_TRY(a->alloc(&a->applied, 1, CandleDqn::AGENT));
        // the library's own seeded initialiser, uniform(+-1/sqrt(fan_in)) per layer (tests set parameters)
        std::vector<float> ref(a->ref_count(), 0.f);
        const int fan[5] = {64 * cfg->n_stack, 512, 576, 3136, 512}, outs[5] = {32, 64, 64, 512, c.n_actions};
        float* q = ref.data();
        for (int l = 0; l < 5; ++l) {
            const int u[1] = {1};
            const MlpLayout one = make_mlp(fan[l], u, 0, outs[l], false);
            mlp_init_reference(one, c.seed * 7 + 1 + (uint64_t)l, q);
            q += one.ref_total;
        }
        BDR_TRY(a->set_params(0, ref.data(), ref.size()));
        BDR_TRY(a->set_params(1, ref.data(), ref.size()));   // track(qnet_tgt, qnet, 1.0) (dqn/base.rs:251)
        return a->ensure_batch((int)c.batch_size);
    }();
    if (st != BDR_OK) { delete a; return st; }
    *out = a;
    return BDR_OK;
}

int32_t bdr_candle_dqn_cnn_update_on_batch(bdr_agent* base, uint64_t n, const uint8_t* obs, const int64_t* act, const uint8_t* next_obs, const float* reward,
                                           const int8_t* term, const int8_t* /*is_truncated: read by nothing, dqn/base.rs:62*/, bdr_dqn_record* rec)
{
    BDR_REQUIRE(base && obs && act && next_obs && reward && term, "null argument");
    BDR_REQUIRE(!strcmp(base->kind(), "candle_dqn") && static_cast<CandleDqn*>(base)->cnn_form(), "not a DQN (candle) agent with the AtariCnn Q-network");
    CandleDqnCnn* a = static_cast<CandleDqnCnn*>(base);
    BDR_REQUIRE(n >= 1 && n <= 65536, "batch size out of range");
    BDR_HIP(hipSetDevice(a->device));
    BDR_TRY(a->ensure_batch((int)n));
    const size_t rb = a->row_bytes();
    if (n > a->u_cap8) {
        BDR_HIP(hipStreamSynchronize(a->stream));
        a->release(CandleDqn::STAGING);
        a->u_cap8 = 0;
        BDR_TRY(a->alloc(&a->u_obs8, n * rb, CandleDqn::STAGING, false)); BDR_TRY(a->alloc(&a->u_next8, n * rb, CandleDqn::STAGING, false));
        BDR_TRY(a->alloc(&a->u_act, n, CandleDqn::STAGING, false)); BDR_TRY(a->alloc(&a->u_rew, n, CandleDqn::STAGING, false));
        BDR_TRY(a->alloc(&a->u_term, round_up(n, 16), CandleDqn::STAGING, false));
        a->u_cap8 = n;
    }
    BDR_HIP(hipMemcpyAsync(a->u_obs8, obs, n * rb, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_next8, next_obs, n * rb, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_act, act, n * 8, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_rew, reward, n * 4, hipMemcpyHostToDevice, a->stream));
    BDR_HIP(hipMemcpyAsync(a->u_term, term, n, hipMemcpyHostToDevice, a->stream));
    const bool track = a->opt_tracks();
    BDR_TRY(a->update_cnn((int)n, a->u_obs8, reinterpret_cast<const uint8_t*>(a->u_act), 8, a->u_next8, a->u_rew, a->u_term, track));
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
    BDR_REQUIRE(!a->cnn_form(), "this DQN (candle) agent has the AtariCnn Q-network: its rows are u8 (bdr_candle_dqn_cnn_update_on_batch)");
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
