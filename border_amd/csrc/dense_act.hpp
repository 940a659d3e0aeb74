// Policy::sample of the DenseAgent agents (IQL, AWAC: util/actor.rs:226-241; BC: bc/base.rs:49-59) in ONE launch:
//   raw observation rows (f32 or float64, host-staged or device rows row_stride bytes apart) -> f32 -> the normaliser's z
//   (obs_norm_z, common.hpp) -> every layer of the Mlp -> the action.
// The layer-by-layer path is a chain of launches that are each a few dependent round trips long (pack, one k_dense_small per
// layer, the sample kernel); for the handful of rows of an acting call the launches are the cost.  Here a workgroup owns a block
// of 32 observation rows and runs every layer for them: the activations stay in LDS in two ping-pong buffers (row stride = the
// stored layer's padded width + 4 floats: the 16 lanes of a ds_read_b128 phase land in different banks, as dense_chain.hpp's h0),
// the weights are read from L2 and not staged.  No workgroup waits for another one - no flags, no tickets: with n up to 65 536
// rows the grid need not be co-resident.
//   Bits.  Every 32 x 32 output tile of every layer is formed by dense_small_tile / dense_small_tile_pre and dense_small_sum
//   (dense.hpp) with the LDS rows as the A operand, then bias and ReLU in dense_small_body's order: the tile k_dense_small forms.
//   DenseAgent's forward always takes k_dense_small (dense_forward_z(..., true)), so the actions have the bits of the
//   layer-by-layer path at every n (tests/test_gpu_dense_act.py asserts == on the raw bits).  The element code of the two
//   epilogues (candle_sample_elem, bc_act_out / bc_argmax, dqn_q_argmax) is shared with k_candle_sample, k_bc_act and k_cdqn_act.
//   Latency.  A tile's weight loads depend on nothing the kernel computes.  TEAMS four-wave teams take TEAMS tiles of a layer per
//   round (wave w of a team: k-slice w of its tile), and each wave fetches the weights and the bias of its NEXT round - also across
//   the layer boundary - before the MFMAs of the current one (dense_small_load_b; layers with a reduction over 256 load inside
//   dense_small_tile instead).  A row block runs on ONE CU: its four matrix pipes bound the pen network (64-256-256-256-64 padded,
//   2 560 MFMAs of 64 cycles) at 17 us whatever n <= 32 is, and all weights pass through that CU's vector-memory path.  Measured
//   (DESIGN.md 14): 40 us at n = 1 against 29 us of kernels on the layer path, whose every layer spreads over eight CUs - the one
//   launch wins from a few hundred rows up, so the path is opt-in (bdr_agent_set_act_path) and the default stays layer by layer.
//   LDS plan (dynamic, floats): buf0 [32][W + 4] | buf1 [32][W + 4] | red [TEAMS][4][32][33], W = the widest padded layer
//   input / output.  TEAMS = 2 when that fits 160 KB (W <= 448), else 1 (W <= 512: 148 992 bytes); wider networks keep the layer path.
//   Bounds.  rows: block row r is read from memory only for m0 + r < n and column c < O, and stored (out / idx) only for
//   m0 + r < n; LDS rows r >= n - m0 are zero.  LDS: r < 32, c < Kp or Np <= W.  Weights: k < Kp, column < Np of the layer
//   (t < Np / 32).  out: (m0 + r) * A + j < n * A; idx: m0 + r < n.  mean / std: c < O = the normaliser's dim (checked by the host).
//   A group.  The body is a function, dense_act_body: k_dense_act runs it on its argument struct, k_bc_act_group (bc_group.hpp) and
//   k_candle_act_group (candle_act_group.hpp) on args[member] and calls[member] of a group with the member as grid dimension y - P
//   members with a row each are P workgroups on P CUs in one launch, the form this kernel has anyway.
#pragma once

namespace bdr {
namespace candle {

// counter-based N(0,1) of the agent's noise stream (the same generator as SAC's: splitmix64 hash -> Box-Muller)
__device__ __forceinline__ float randn_at(uint64_t seed, uint64_t counter, size_t i)
{
    uint64_t x = (seed + 0x9E3779B97F4A7C15ull) ^ ((counter + i + 1) * 0xBF58476D1CE4E5B9ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    const float u1 = ((float)(x >> 40) + 1.0f) * (1.0f / 16777217.0f);
    const float u2 = (float)((x >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

}  // namespace candle
}  // namespace bdr

namespace {
using namespace bdr;

// ---- the element code of Policy::sample, shared by the layer path's kernels and k_dense_act -----------------------------------
// GaussianActor (util/actor.rs:226-241): train: mean + exp(clamp(l)) z, eval: mean; then clamp or scale * tanh.  l = head2[j]
// (Mlp3) or, with mlp2 set, exp(s) of the row's own s (Mlp2, mlp2.rs:41: the double exponential is the reference's).  z = the host
// draw z[t] when given, else the device stream at counter + t (t = b * A + j).
struct SampleElem {
    const float* head2; float lo, hi; int tanh_limit; float amin, amax, scale;
    int train; uint64_t seed, counter; const float* z;
    int mlp2;
};
__device__ __forceinline__ float candle_sample_elem(const SampleElem& p, float a, int j, size_t t, float s = 0.f)
{
#pragma clang fp contract(off)
    if (p.train) {
        const float l = p.mlp2 ? expf(s) : p.head2[j];
        const float sd = expf(fminf(fmaxf(l, p.lo), p.hi));
        const float zz = p.z ? p.z[t] : candle::randn_at(p.seed, p.counter, t);
        const float e = sd * zz;
        a = e + a;
    }
    if (p.tanh_limit) { const float th = tanhf(a); a = p.scale * th; }
    else a = fminf(fmaxf(a, p.amin), p.amax);
    return a;
}
// BC (bc/base.rs:49-59): Continuous = act_out(z); Discrete = argmax_j act_out(z[j]), the lowest index among equal values
__device__ __forceinline__ float bc_act_out(int kind, float z)
{
    if (kind == BDR_ACTIVATION_RELU) return z > 0.f ? z : 0.f;
    if (kind == BDR_ACTIVATION_TANH) return tanhf(z);
    if (kind == BDR_ACTIVATION_SIGMOID) return 1.f / (1.f + expf(-z));
    return z;
}
__device__ __forceinline__ int bc_argmax(int kind, const float* z, int A)
{
    int best = 0;
    float bv = bc_act_out(kind, z[0]);
    for (int j = 1; j < A; ++j) {
        const float v = bc_act_out(kind, z[j]);
        if (v > bv) { bv = v; best = j; }
    }
    return best;
}

// the candle DQN (dqn/base.rs:103, :108, :226): argmax over a row of action values, the output activation already applied by the
// last layer.  bc_argmax's rule: the lowest index among equal values; a NaN never wins a comparison, so a row whose first value is
// NaN answers 0 and a NaN elsewhere is passed over.
__device__ __forceinline__ int dqn_q_argmax(const float* q, int A) { return bc_argmax(BDR_ACTIVATION_NONE, q, A); }

// ---- the layer path's prologue for raw rows: out[k][c] = z((float)rows[k][c]) (norm given) or (float)rows[k][c], contiguous f32 rows
template <typename T>
__global__ __launch_bounds__(256) void k_act_raw_rows(const uint8_t* __restrict__ rows, unsigned long long row_stride, unsigned long long n, int O,
                                                      const float* __restrict__ mean, const float* __restrict__ std, float* __restrict__ out)
{
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * (unsigned long long)O) return;
    const unsigned long long k = e / O; const int c = (int)(e % O);
    float x = (float)reinterpret_cast<const T*>(rows + k * row_stride)[c];
    if (mean) x = obs_norm_z(x, mean[c], std[c]);
    out[e] = x;
}

// ---- k_dense_act --------------------------------------------------------------------------------------------------------------
constexpr int DA_MAX_LAYERS = BDR_MAX_UNITS + 1;
constexpr int DA_MAX_W = 512;
constexpr size_t DA_LDS_MAX = 160 * 1024;
enum { DA_CANDLE = 0, DA_BC = 1, DA_BC_DISCRETE = 2, DA_DQN = 3 };
inline size_t dense_act_lds(int W, int teams) { return ((size_t)2 * 32 * (W + 4) + (size_t)teams * 4 * 32 * 33) * sizeof(float); }

struct DenseActLayer { const float* w; const float* b; int Kp, Np, relu; };
struct DenseActArgs {
    const uint8_t* rows; unsigned long long row_stride; int f64;   // row k at rows + k * row_stride, O elements of f32 / float64
    int n, O, A, nl, W;
    const float* mean; const float* std;                           // the normaliser's f32 statistics [O], or null
    DenseActLayer L[DA_MAX_LAYERS];
    int mode, kind;                                                // DA_*; BC: activation_out
    SampleElem e;                                                  // DA_CANDLE
    float* out; long long* idx;                                    // [n][A] actions (DA_CANDLE, DA_BC); [n] (DA_BC_DISCRETE); both (DA_DQN)
};

// "these loaded registers have landed": the wait is HERE, before the next round's loads are issued behind them (dense_chain.hpp chain_land)
__device__ __forceinline__ void dense_act_land(const f32x4 (&v)[8], const f32x4& b)
{
    asm volatile("" ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]), "v"(b));
}

// the candle DQN's epilogue (dqn/base.rs:203), once for DA_EPI_ALL's DA_DQN branch and for DA_EPI_DQN: the Q rows themselves - the
// last layer's rows in LDS without their padding - and each row's first maximum (dqn_q_argmax).  Bounds: rr < rows_here <= 32,
// j < A <= ld - 4; out at (m0 + rr) * A + j, idx at m0 + tid, both below the call's n rows.
template <int NTHR>
__device__ __forceinline__ void dense_act_dqn_rows(const float* cur, int ld, int A, int m0, int rows_here, int tid, float* out, long long* idx)
{
    for (int e = tid; e < rows_here * A; e += NTHR) {
        const int rr = e / A, j = e % A;
        out[(size_t)(m0 + rr) * A + j] = cur[rr * ld + j];
    }
    if (tid < rows_here) idx[m0 + tid] = dqn_q_argmax(cur + tid * ld, A);
}

// The body of k_dense_act and of the group entry k_bc_act_group (bc_group.hpp).  `a`: the network and the epilogue (layers, widths,
// mode, kind, A, O, W); `call`: the words of this call (rows, row_stride, f64, n, mean, std, out, idx).  The standalone kernel passes
// its one argument struct as both; the group entry passes a member's entries of two arrays it reads in place through the constant
// address space, so Args and Call are template parameters and a layer is copied field by field (a struct copy would have to bind a
// generic reference to the constant address space).  EPI: the epilogues the entry instantiates.
//   DA_EPI_ALL     k_dense_act: every mode; DA_BC_DISCRETE and DA_DQN leave the kernel early, DA_CANDLE reads a.e as it stands.
//   DA_EPI_BC      the caller has refused every mode but DA_BC: bc_act_out alone, every thread returns to the entry.
//   DA_EPI_CANDLE  the caller has refused every mode but DA_CANDLE: candle_sample_elem on a SampleElem built in registers, field by
//                  field - the static words (head2, the clamps, the limit, seed, mlp2) from a.e, the words of this call (train,
//                  counter) from `call`, z null: the draw of element t = (m0 + rr) * A + j of the member's own call is counter + t,
//                  the one the member's own kernel takes.  Every thread returns to the entry.
//   DA_EPI_DQN     the caller has refused every mode but DA_DQN (k_cdqn_act_group, candle_dqn_group.hpp): the Q rows and each row's
//                  first maximum, as DA_EPI_ALL's DA_DQN branch writes them; every thread returns to the entry.
enum { DA_EPI_ALL = 0, DA_EPI_BC = 1, DA_EPI_CANDLE = 2, DA_EPI_DQN = 3 };
template <int TEAMS, int EPI, class Args, class Call>
__device__ __forceinline__ void dense_act_body(const Args& a, const Call& call, float* da_lds)
{
    constexpr int NTHR = 256 * TEAMS;
    const int S = 32 * (a.W + 4);
    float* cur = da_lds;
    float* nxt = da_lds + S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), team = wv >> 2, wave = wv & 3;
    float (*red)[32][33] = reinterpret_cast<float (*)[32][33]>(da_lds + 2 * (size_t)S + (size_t)team * 4 * 32 * 33);
    const int m0 = (int)blockIdx.x * 32;
    const int rows_here = min(32, call.n - m0);
    const int r = (tid & 255) >> 3, c4 = (tid & 7) * 4;   // the thread's element quad of its team's tile (dense_small_body's)

    // the first round's weights and bias: they depend on nothing, issued before the rows are read
    f32x4 bv[8], bvn[8], bias = {0.f, 0.f, 0.f, 0.f}, biasn = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) { bv[q] = f32x4{0.f, 0.f, 0.f, 0.f}; bvn[q] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    {
        const auto& l0 = a.L[0];
        if (team * 32 < l0.Np) {
            bias = *reinterpret_cast<const f32x4*>(l0.b + team * 32 + c4);
            if (l0.Kp <= 256) dense_small_load_b<false>(l0.w, l0.Np, team * 32, l0.Kp, wave, lane, bv);
        }
    }
    // ---- prologue: rows -> f32 -> z -> LDS, zero-padded to Kp; rows >= n of the last block are zero
    {
        const int Kp0 = a.L[0].Kp, ld0 = Kp0 + 4;
        for (int e = tid; e < 32 * Kp0; e += NTHR) {
            const int rr = e / Kp0, c = e % Kp0;
            float x = 0.f;
            if (rr < rows_here && c < a.O) {
                const uint8_t* row = call.rows + (size_t)(m0 + rr) * call.row_stride;
                x = call.f64 ? (float)reinterpret_cast<const double*>(row)[c] : reinterpret_cast<const float*>(row)[c];
                if (call.mean) x = obs_norm_z(x, call.mean[c], call.std[c]);
            }
            cur[rr * ld0 + c] = x;
        }
    }
    __syncthreads();

    // ---- the layers: TEAMS tiles per round
    for (int l = 0; l < a.nl; ++l) {
        DenseActLayer ly;
        ly.w = a.L[l].w; ly.b = a.L[l].b; ly.Kp = a.L[l].Kp; ly.Np = a.L[l].Np; ly.relu = a.L[l].relu;
        const int ldi = ly.Kp + 4, ldo = ly.Np + 4, NT = ly.Np / 32;
        const float* arow = cur + (lane & 31) * ldi;
        const bool pre = ly.Kp <= 256;
        for (int t0 = 0; t0 < NT; t0 += TEAMS) {
            const int t = t0 + team;   // wave-uniform
            dense_act_land(bv, bias);
            // the next round's operands (the next tiles of this layer, or the first of the next layer)
            {
                int ln = l, tn = t0 + TEAMS;
                if (tn >= NT) { ln = l + 1; tn = 0; }
                tn += team;
                if (ln < a.nl) {
                    const auto& lx = a.L[ln];
                    if (tn * 32 < lx.Np) {
                        biasn = *reinterpret_cast<const f32x4*>(lx.b + tn * 32 + c4);
                        if (lx.Kp <= 256) dense_small_load_b<false>(lx.w, lx.Np, tn * 32, lx.Kp, wave, lane, bvn);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise sink the loads to their use in the next round)
            if (t < NT) {
                auto loadA = [&](int k) { return *reinterpret_cast<const f32x4*>(arow + k); };
                if (pre) dense_small_tile_pre(loadA, bv, ly.Kp, wave, lane, red);
                else dense_small_tile<false>(loadA, ly.w, ly.Np, t * 32, ly.Kp, wave, lane, red);
            }
            __syncthreads();
            if (t < NT) {
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) { v[q] = dense_small_sum(red, r, c4 + q); v[q] += bias[q]; if (ly.relu) v[q] = v[q] > 0.f ? v[q] : 0.f; }
                *reinterpret_cast<f32x4*>(nxt + r * ldo + t * 32 + c4) = v;
            }
            __syncthreads();   // red is the next round's; the layer's output is complete before the next layer reads it
#pragma unroll
            for (int q = 0; q < 8; ++q) bv[q] = bvn[q];
            bias = biasn;
        }
        float* s = cur; cur = nxt; nxt = s;
    }

    // ---- epilogue: the last layer's rows [32][Np + 4] in cur -> actions
    const int ldz = a.L[a.nl - 1].Np + 4;
    if constexpr (EPI == DA_EPI_ALL) {
        if (a.mode == DA_BC_DISCRETE) {
            if (tid < rows_here) call.idx[m0 + tid] = bc_argmax(a.kind, cur + tid * ldz, a.A);
            return;
        }
        if (a.mode == DA_DQN) {
            dense_act_dqn_rows<NTHR>(cur, ldz, a.A, m0, rows_here, tid, call.out, call.idx);
            return;
        }
    }
    if constexpr (EPI == DA_EPI_DQN) {
        dense_act_dqn_rows<NTHR>(cur, ldz, a.A, m0, rows_here, tid, call.out, call.idx);
    } else if constexpr (EPI == DA_EPI_CANDLE) {
        SampleElem se;   // field by field: static indices, registers
        se.head2 = a.e.head2; se.lo = a.e.lo; se.hi = a.e.hi; se.tanh_limit = a.e.tanh_limit; se.amin = a.e.amin; se.amax = a.e.amax; se.scale = a.e.scale;
        se.seed = a.e.seed; se.mlp2 = a.e.mlp2;
        se.train = call.train; se.counter = call.counter; se.z = nullptr;
        for (int e = tid; e < rows_here * a.A; e += NTHR) {
            const int rr = e / a.A, j = e % a.A;
            const size_t t = (size_t)(m0 + rr) * a.A + j;
            const float z = cur[rr * ldz + j];
            call.out[t] = candle_sample_elem(se, z, j, t, se.mlp2 ? cur[rr * ldz + a.A + j] : 0.f);
        }
    } else {
        for (int e = tid; e < rows_here * a.A; e += NTHR) {
            const int rr = e / a.A, j = e % a.A;
            const size_t t = (size_t)(m0 + rr) * a.A + j;
            const float z = cur[rr * ldz + j];
            if constexpr (EPI == DA_EPI_BC) call.out[t] = bc_act_out(a.kind, z);
            else call.out[t] = a.mode == DA_CANDLE ? candle_sample_elem(a.e, z, j, t, a.e.mlp2 ? cur[rr * ldz + a.A + j] : 0.f) : bc_act_out(a.kind, z);
        }
    }
}

template <int TEAMS>
__global__ __launch_bounds__(256 * TEAMS) void k_dense_act(DenseActArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float da_lds[];
    dense_act_body<TEAMS, DA_EPI_ALL>(a, a, da_lds);
}

}  // namespace
