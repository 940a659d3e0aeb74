// The head forward of the candle DQN's AtariCnn Q-network in its split-k form (BDR_HEAD_FORM_SPLITK): l1 (3136 -> 512, + b1, ReLU)
// and l2 (512 -> A, + b2) of ALL instances of an update - (p, obs), (p_tgt, next_obs) and, double_dqn, (p, next_obs) - and of all
// row tiles in ONE launch, k_cdqn_head_fwd, in place of the two k_dense_small launches of the layer form.
//
// Why.  k_dense_small gives l1 ceil(B / 32) * 16 tiles per instance: 32 workgroups at B = 32 with two instances, each wave walking
// 784 k = 392 dependent MFMAs fed straight from global memory, on a 256-CU machine.  Here l1 is cut as k_cnn_act_head cuts it for one
// acting tile (cnn_act_img.hpp), for any B and every instance:
//   grid (16, CHF_KS, nz * row_tiles), 256 threads: blockIdx.x = column tile nt of l1 (32 columns), blockIdx.y = k-slice ks of
//   CHF_KSL = 448 k, blockIdx.z = zt = z * row_tiles + rt (instance z < nz <= 3, row tile rt of 32 rows).  Wave w multiplies the
//   sub-slice of 112 k = 7 x 16 of ONE 32 x 32 tile (dense_small_tile<false>: 28 dependent MFMAs), the four sub-slices meet in LDS
//   (dense_small_sum) and the partial tile goes to part[zt][ks] with agent-scope stores.  224 workgroups at B = 32, nz = 2.
//   counter (zt, nt)   taken behind the partial's stores; the LAST of the CHF_KS arrivers loads the seven partials of its 32 x 32 tile
//                      (16-byte loads served by the coherent level, all in flight before the one wait), adds them in slice order
//                      ((((((p0 + p1) + p2) + p3) + p4) + p5) + p6), adds b1, applies ReLU and stores h1 rows < B into the instance's
//                      layer-0 activation buffer - the buffer l2's weight gradient and l2's input-gradient mask read.
//   counter (zt, 16)   taken behind those h1 stores; the LAST of the 16 column tiles' arrivers requests b2 and the first tile of W2,
//                      stages the row tile's 32 h1 rows in LDS (hs[32][516]) and runs l2 one 32-column tile at a time over the whole
//                      padded width ld2 (kred 512, dense_small_tile's k-slots and MFMA order from LDS rows; the next tile's W2 is
//                      requested as soon as the current one has been multiplied), + b2, into the instance's last activation buffer
//                      with the row stride ld2: every element the two k_dense_small launches write, this launch writes.
// No workgroup waits for another one and there is no fence: a counter is taken once, behind the workgroup's own agent-scope stores
// (dense.hpp last_workgroup: s_waitcnt, barrier, agent-scope fetch-add); whoever takes the last ticket goes on and re-arms the
// counter, so the counters are zero between launches and the grid need not be co-resident.
// W2 and b2 cannot be requested before the l1 tile: only one workgroup in 16 x CHF_KS multiplies l2, and which one is known when the
// second ticket is taken.  b1 is requested before the l1 tile by every workgroup (one 16-byte load), W2 / b2 before h1 is staged.
//
// Summation order.  CHF_KS and the cut are constants, the same for every B, nz and row: an h1 element is the seven slice sums added in
// slice order, each the four wave sub-slices added as dense_small_sum adds them, each one f32 accumulator over its 112 k ascending;
// a q element is l2's four wave slices of 128 k.  Nothing depends on the row's position in the batch, on B, or on the instance:
// acting (one instance) and the update's forward give a row the same bits.  h1 differs from the layer form's in rounding (seven
// slices here, one there); q from the SAME h1 is the layer form's to the bit.
//
// Bounds (B >= 1, row_tiles = ceil(B / 32), zt < nz * row_tiles, m0 = 32 rt).
//   x[z]     rows min(m0 + (lane & 31), B - 1) < B, floats 448 ks + k, k < 448: < 3136 (rows >= B alias row B - 1, never stored)
//   w1[z]    rows 448 ks + k < 3136, columns 32 nt + i < 512;   b1[z] at 32 nt + c4 ... + 3 < 512
//   part     ((zt * CHF_KS + ks) * 32 + r) * 512 + 32 nt + c4 + q, r < 32: below nz * row_tiles * CHF_KS * 32 * 512 floats; written
//            and read at rows m0 + r < B only
//   counters zt * CHF_COUNTERS + nt (nt < 16) and + 16: below nz * row_tiles * CHF_COUNTERS words
//   h1[z]    written at rows m0 + r < B, columns 32 nt + c4 + q < 512 (row stride 512); read at rows min(m0 + row, B - 1), row < 32
//   hs       vector x = tid + 256 e < 4096: row x >> 7 < 32, floats 4 (x & 127) ... + 3 < 512 of 516;  l2 reads hs[lane & 31][k], k < 512
//   w2[z]    rows k < 512, columns t0 + i, t0 + 32 <= ld2 (ld2 % 64 == 0);   b2[z] at t0 + c4 ... + 3 < ld2 (the padded bias)
//   q[z]     rows m0 + r < B, columns t0 + c4 ... + 3 < ld2 (row stride ld2)
//   red      [4][32][33]: dense_small_tile writes [wave][row < 32][i < 32]
// LDS: red 16 896 + hs 66 048 + 4 bytes: one workgroup per CU.
// The kernel is compiled in a translation unit of its own (cdqn_head_fwd.hip defines BDR_CDQN_HEAD_FWD_KERNELS): candle_dqn.hip sees
// the argument struct and the launcher, and every kernel it held before keeps its registers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace bdr {

constexpr int CHF_KS = 7;                 // k-slices of l1
constexpr int CHF_KSL = 3136 / CHF_KS;    // 448 k each: four wave sub-slices of 112 = 7 x 16
constexpr int CHF_COUNTERS = 17;          // per (instance, row tile): one per column tile of l1, one for the row tile
constexpr int CHF_MAX_Z = 3;
static_assert(CHF_KSL * CHF_KS == 3136 && CHF_KSL % 64 == 0, "dense_small_tile wants kred % 64 == 0");

inline int chf_row_tiles(int B) { return (B + 31) / 32; }
inline size_t chf_part_floats(int nz, int B) { return (size_t)nz * chf_row_tiles(B) * CHF_KS * 32 * 512; }
inline size_t chf_counter_words(int nz, int B) { return (size_t)nz * chf_row_tiles(B) * CHF_COUNTERS; }

struct CdqnHeadFwdArgs {
    const float* x[CHF_MAX_Z];                          // conv3's output rows [B][3136], (h, w, c) order
    const float *w1[CHF_MAX_Z], *b1[CHF_MAX_Z];         // l1: [3136][512], [512]
    const float *w2[CHF_MAX_Z], *b2[CHF_MAX_Z];         // l2: [512][ld2], [ld2]
    float *h1[CHF_MAX_Z], *q[CHF_MAX_Z];                // [B][512], [B][ld2]
    float* part;                                        // chf_part_floats(nz, B)
    unsigned* counters;                                 // chf_counter_words(nz, B), zero between launches
    int B, ld2, row_tiles;
};

hipError_t launch_cdqn_head_fwd(hipStream_t st, int nz, const CdqnHeadFwdArgs& a);   // grid (16, CHF_KS, nz * row_tiles)

}  // namespace bdr

#ifdef BDR_CDQN_HEAD_FWD_KERNELS
#include "dense.hpp"

namespace bdr {

// The B operands of l2's tile n0 for this wave: its 128 k of kred = 512 as eight 16-wide chunks, in dense_small_tile's k-slots
__device__ __forceinline__ void chf_load_w2(const float* __restrict__ w, int ld, int n0, int wave, int lane, f32x4 (&bv)[16])
{
    const int i = lane & 31, h = lane >> 5;
    const float* wcol = w + n0 + i;
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float* p = wcol + (size_t)(128 * wave + 16 * c + 8 * u + 4 * h) * ld;
            bv[c * 2 + u] = f32x4{p[0], p[ld], p[2 * (size_t)ld], p[3 * (size_t)ld]};
        }
}
// dense_small_tile<false> at kred = 512 with the B operands fetched ahead and the A rows in LDS: same k-slots, same MFMA order, same bits
__device__ __forceinline__ void chf_l2_tile(const float* hrow, const f32x4 (&bv)[16], int wave, int lane, float (*red)[32][33])
{
    const int i = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(hrow + 128 * wave + 16 * c + 8 * u + 4 * h);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[c * 2 + u][q], acc, 0, 0, 0);
        }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][(r & 3) + 8 * (r >> 2) + 4 * h][i] = acc[r];
}

static __global__ __launch_bounds__(256) void k_cdqn_head_fwd(CdqnHeadFwdArgs a)
{
    __shared__ float red[4][32][33];
    __shared__ __attribute__((aligned(16))) float hs[32][516];
    __shared__ unsigned s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = blockIdx.x, ks = blockIdx.y, zt = blockIdx.z, z = zt / a.row_tiles, m0 = (zt - z * a.row_tiles) * 32;
    const int n0 = nt * 32, k0 = ks * CHF_KSL;
    const float* arow = a.x[z] + (size_t)min(m0 + (lane & 31), a.B - 1) * 3136 + k0;   // rows >= B alias the last row (never stored)
    const int r = tid >> 3, c4 = (tid & 7) * 4, col = n0 + c4, m = m0 + r;
    const f32x4 bv1 = *reinterpret_cast<const f32x4*>(a.b1[z] + col);   // the epilogue's operand, requested beside the tile operands
    dense_small_tile<false>([&](int k) { return *reinterpret_cast<const f32x4*>(arow + k); }, a.w1[z] + (size_t)k0 * 512, 512, n0, CHF_KSL, wave, lane, red);
    __syncthreads();
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = dense_small_sum(red, r, c4 + q);
    float* const part = a.part + (size_t)zt * CHF_KS * 32 * 512;
    if (m < a.B) {
        float* p = part + ((size_t)ks * 32 + r) * 512 + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) st_agent(p + q, v[q]);
    }
    unsigned* const counters = a.counters + (size_t)zt * CHF_COUNTERS;
    if (!last_workgroup(counters + nt, (unsigned)CHF_KS, &s_last)) return;

    // ---- the column tile's partials in slice order, whoever arrives last
    float* const h1 = a.h1[z];
    if (m < a.B) {
        const float* p0 = part + (size_t)r * 512 + col;
        f32x4 t[CHF_KS];
#pragma unroll
        for (int e = 0; e < CHF_KS; ++e) {
            const float* ps = p0 + (size_t)e * 32 * 512;
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(t[e]) : "v"(ps) : "memory");
        }
        static_assert(CHF_KS == 7, "the wait below names seven destinations");
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]) :: "memory");
        v = t[0];
#pragma unroll
        for (int e = 1; e < CHF_KS; ++e) v += t[e];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = v[q] + bv1[q];
            st_agent(h1 + (size_t)m * 512 + col + q, x > 0.f ? x : 0.f);   // read by the workgroup below, possibly on another XCD
        }
    }
    if (!last_workgroup(counters + 16, 16u, &s_last)) return;

    // ---- l2 of this row tile, by the workgroup that completed its last column tile
    const float* const w2 = a.w2[z];
    f32x4 wv[16];
    chf_load_w2(w2, a.ld2, 0, wave, lane, wv);   // in flight while h1 is staged
    for (int e0 = 0; e0 < 16; e0 += 8) {         // h1 -> LDS (rows >= B: a copy of row B - 1)
        f32x4 t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int x = tid + 256 * (e0 + e);   // 16-byte vector x of hs: row x >> 7, floats 4 (x & 127) ...
            const float* ps = h1 + (size_t)min(m0 + (x >> 7), a.B - 1) * 512 + 4 * (x & 127);
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(t[e]) : "v"(ps) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]) :: "memory");
#pragma unroll
        for (int e = 0; e < 8; ++e) { const int x = tid + 256 * (e0 + e); *reinterpret_cast<f32x4*>(&hs[x >> 7][4 * (x & 127)]) = t[e]; }
    }
    __syncthreads();
    const float* hrow = hs[lane & 31];
    float* const qrow = a.q[z] + (size_t)min(m, a.B - 1) * a.ld2 + c4;
    for (int t0 = 0; t0 < a.ld2; t0 += 32) {
        const f32x4 bv2 = *reinterpret_cast<const f32x4*>(a.b2[z] + t0 + c4);
        chf_l2_tile(hrow, wv, wave, lane, red);
        if (t0 + 32 < a.ld2) chf_load_w2(w2, a.ld2, t0 + 32, wave, lane, wv);   // the next tile's weights, across the barrier and the stores
        __syncthreads();
        if (m < a.B) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = dense_small_sum(red, r, c4 + q) + bv2[q];
            *reinterpret_cast<f32x4*>(qrow + t0) = v;
        }
        __syncthreads();   // red is free again
    }
}

hipError_t launch_cdqn_head_fwd(hipStream_t st, int nz, const CdqnHeadFwdArgs& a)
{
    return step_launch(st, false, k_cdqn_head_fwd, dim3(16, CHF_KS, (unsigned)(nz * a.row_tiles)), dim3(256), a);
}

}  // namespace bdr
#endif  // BDR_CDQN_HEAD_FWD_KERNELS
