// The head backward of the candle DQN's AtariCnn Q-network in its fused form (BDR_HEAD_BWD_FUSED): l2's input gradient dh1, l1's
// input gradient dy3 under conv3's ReLU mask, and the weight-gradient partials of l1 and l2 in ONE launch, k_cdqn_head_bwd, in place
// of the two k_dense_small<true> launches and k_dense_dw_small_group of the layer form.  k_dense_reduce_adam and the conv trunk's
// backward run behind it as they were: the launch writes every element those three write, into the same buffers.
//
// Why.  At B = 32 the three launches are under-filled grids (16 tiles, 98 tiles, then 1 600 workgroups of four MFMAs per wave), each
// paying a launch boundary and first-touch latency for about 0.3 GFLOP together.  dh1[b][j] = [h1[b][j] > 0] sum_a dq[b][a] W2[j][a]
// is A <= 32 terms per element, so every workgroup that needs dh1 forms it itself instead of waiting for a launch that stores it.
//   grid x = CHB_KT + 16 * (ld2 / 32), 256 threads.
//   blockIdx.x = kt < CHB_KT = 98: the 32 feature rows kt of W1 (3136 = 98 x 32).  The workgroup requests its W1 operands (per lane 16
//     float4 of row 32 kt + (lane & 31): wave w's 128 k of dense_small_tile<true>) and W2's A columns (staged transposed, w2s[a][512]),
//     then walks the batch's row tiles rt of 32 rows IN ORDER.  Per row tile:
//       stage   dq rows (dqs[32][32], rows >= B zero) and the a3 tile (a3s[32][33], rows >= B alias row B - 1)
//       dh1     thread t forms columns 4 (t & 127) ... + 3 of rows (t >> 7) + 2 e, e < 16: an fmaf chain over a = 0 ... A - 1 ascending
//               from w2s and dqs (a broadcast read), masked by h1 > 0, into dhs[32][516].  Rows >= B are exactly zero (their dq is).
//       (a)     dW1[32 kt + i][n] += sum_b a3[b][32 kt + i] dh1[b][n] on v_mfma_f32_32x32x2_f32: wave w owns the column tiles 4 w ... 4 w + 3,
//               MFMA g < 16 of a tile takes rows 2 g and 2 g + 1; the four accumulators stay in registers across ALL row tiles.
//       (b)     dy3[b][32 kt + c] = [a3 > 0] sum_j dh1[b][j] W1[32 kt + c][j]: dense_small_tile<true>'s k-slots and MFMA order at kred = 512
//               with the A rows in LDS and the B operands fetched at kernel start; the four wave slices meet in red (dense_small_sum).
//       The workgroup kt == rt stores the row tile's dh1 rows < B into dy[0]; the workgroup kt == CHB_KT - 1 adds the tile's column
//       sums to its db1 registers (thread t: columns 2 t, 2 t + 1).
//     Behind the walk: the four accumulators -> l1's chunk-0 partial rows 32 kt ... + 31; workgroup CHB_KT - 1 -> the bias row.
//   blockIdx.x >= CHB_KT: one 32 x 32 tile of dW2 = h1^T dq (and, in the tiles of k-tile 0, db2): k_dense_dw_small_group's tile for one
//     chunk - the same rows per wave, k-slots and combine, so l2's partials are the layer form's to the bit.
// No workgroup waits for another one, there are no partial sums through memory, no tickets, no counters, nothing to re-arm.
//
// Summation order: a function of B and the constants only.  dh1: a ascending.  dW1: one f32 accumulator over b ascending, two rows
// per MFMA.  db1: per row tile ((p0 + p1) + (p2 + p3)), p_k = rows 8 k ... 8 k + 7 ascending, the tiles added in order.  dy3:
// dense_small_tile<true>'s.  dW2, db2: k_dense_dw_small_group's.  With dq one-hot per row (k_cdqn_td) dh1 is one rounded product, the
// layer form's bits, and so are dy3 and everything behind it; dW1 and db1 differ from the layer form in rounding from 17 rows up.
//
// Bounds (1 <= B <= CHB_MAX_B, row_tiles = ceil(B / 32), m0 = 32 rt, 1 <= A <= CHB_MAX_A = 32 <= ld2, ld2 % 64 == 0).
//   w1      rows 32 kt + (lane & 31) < 3136, floats 128 w + 16 c + 8 u + 4 h ... + 3 < 512
//   w2      rows t, t + 256 < 512, floats a4 ... a4 + 3, a4 < A rounded up to 4 <= 32 <= ld2
//   w2s     [a < 32][j < 512];  dqs [r < 32][a < 32];  a3s [r < 32][c < 32 of 33];  dhs [r < 32][j < 512 of 516];  red [4][32][33];  bred [4][32]
//   dq      rows min(m0 + r, B - 1) < B, floats 4 (t & 7) ... + 3 < 32 <= ld2;  dW2 tiles: rows < B, columns 32 nt2 + i < ld2
//   h1      rows min(m0 + r, B - 1) < B, floats 4 (t & 127) ... + 3 < 512;      dW2 tiles: rows < B, columns 32 kt2 + i < 512
//   a3      rows min(m0 + r, B - 1) < B, floats 32 kt + 4 (t & 7) ... + 3 < 3136
//   dh1     written at rows m0 + r < B, floats 4 (t & 127) ... + 3 < 512 (row stride 512)
//   dy3     written at rows m0 + r < B, floats 32 kt + 4 (t & 7) ... + 3 < 3136 (row stride 3136)
//   part1   (32 kt + row) * 512 + col, row < 32, col < 512: < 3136 * 512; the bias row 3136 * 512 + 2 t ... + 1 < 3136 * 512 + 512
//   part2   (32 kt2 + r) * ld2 + 32 nt2 + c, kt2 < 16, nt2 < ld2 / 32: < 512 ld2; the bias row 512 ld2 + 32 nt2 + t, t < 32: < 512 ld2 + ld2
// LDS: dhs 66 048 + w2s 65 536 + red 16 896 + a3s 4 224 + dqs 4 096 + bred 512 = 157 312 bytes: one workgroup per CU.
// The kernel is compiled in a translation unit of its own (cdqn_head_bwd.hip defines BDR_CDQN_HEAD_BWD_KERNELS): candle_dqn.hip sees
// the argument struct and the launcher, and every kernel it held before keeps its registers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace bdr {

constexpr int CHB_KT = 3136 / 32;     // feature-row tiles of W1
constexpr int CHB_MAX_B = 256;        // one dW chunk (DenseAgent::chunks_for), eight row tiles walked by every workgroup
constexpr int CHB_MAX_A = 32;         // W2's columns staged in LDS
static_assert(CHB_KT * 32 == 3136 && CHB_MAX_B / 32 <= CHB_KT, "a workgroup per row tile stores dh1");

struct CdqnHeadBwdArgs {
    const float *dq, *h1, *a3;        // [B][ld2] (k_cdqn_td's output gradient), [B][512], [B][3136]
    const float *w1, *w2;             // the online l1 [3136][512] and l2 [512][ld2]
    float *dh1, *dy3;                 // [B][512], [B][3136]
    float *part1, *part2;             // chunk 0 of the dW partials: l1 [3136 * 512 + 512], l2 [512 * ld2 + ld2]
    int B, ld2, A, row_tiles;
};

hipError_t launch_cdqn_head_bwd(hipStream_t st, const CdqnHeadBwdArgs& a);   // grid CHB_KT + 16 * (ld2 / 32)

}  // namespace bdr

#ifdef BDR_CDQN_HEAD_BWD_KERNELS
#include "dense.hpp"

namespace bdr {

// One 32 x 32 tile of dW2 (rows 32 kt2 ... of h1's columns, columns 32 nt2 ... of dq) over all B rows: dense_dw_small_group_body at one chunk
__device__ __forceinline__ void chb_dw2_tile(const CdqnHeadBwdArgs& a, int tile, float (*red)[32][33], float (*bred)[32])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NT = a.ld2 / 32, kt2 = tile / NT, nt2 = tile % NT;
    const int i = lane & 31, h = lane >> 5;
    const int per_wave = (a.B + 31) / 32 * 8;                 // a quarter of the rows rounded up to 32: a multiple of 8
    const int w0 = wave * per_wave, w1 = min(a.B, w0 + per_wave);
    const float* xcol = a.h1 + kt2 * 32 + i;
    const float* ycol = a.dq + nt2 * 32 + i;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bsum = 0.f;
    for (int rb = w0; rb < w1; rb += 32) {                    // at most two batches of 32 rows (B <= 256)
        float av[4][4], bv[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = rb + 8 * u + 4 * h + s;
                const bool ok = row < w1;
                const int rc = min(row, a.B - 1);
                const float xa = xcol[(size_t)rc * 512], ya = ycol[(size_t)rc * a.ld2];
                av[u][s] = ok ? xa : 0.f; bv[u][s] = ok ? ya : 0.f;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][s], bv[u][s], acc, 0, 0, 0);
                bsum += bv[u][s];
            }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][(r & 3) + 8 * (r >> 2) + 4 * h][i] = acc[r];
    if (kt2 == 0) {
        bsum += __shfl_xor(bsum, 32);
        if (h == 0) bred[wave][i] = bsum;
    }
    __syncthreads();
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = dense_small_sum(red, r, c4 + q);
    *reinterpret_cast<f32x4*>(a.part2 + (size_t)(kt2 * 32 + r) * a.ld2 + nt2 * 32 + c4) = v;
    if (kt2 == 0 && tid < 32) a.part2[(size_t)512 * a.ld2 + nt2 * 32 + tid] = ((bred[0][tid] + bred[1][tid]) + bred[2][tid]) + bred[3][tid];
}

static __global__ __launch_bounds__(256) void k_cdqn_head_bwd(CdqnHeadBwdArgs a)
{
    __shared__ __attribute__((aligned(16))) float dhs[32][516];
    __shared__ __attribute__((aligned(16))) float w2s[CHB_MAX_A][512];
    __shared__ float red[4][32][33];
    __shared__ float a3s[32][33];
    __shared__ __attribute__((aligned(16))) float dqs[32][CHB_MAX_A];
    __shared__ float bred[4][32];
    if ((int)blockIdx.x >= CHB_KT) { chb_dw2_tile(a, (int)blockIdx.x - CHB_KT, red, bred); return; }

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kt = blockIdx.x, i = lane & 31, h = lane >> 5;
    // ---- b-independent operands first: this wave's 128 k of W1's rows for (b), W2's columns for dh1
    f32x4 bw[16];
    {
        const float* wrow = a.w1 + (size_t)(kt * 32 + i) * 512 + 128 * wave + 4 * h;
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int u = 0; u < 2; ++u) bw[c * 2 + u] = *reinterpret_cast<const f32x4*>(wrow + 16 * c + 8 * u);
    }
    for (int a4 = 0; a4 < a.A; a4 += 4) {                     // (workgroup-uniform; a4 + 3 < 32 <= ld2)
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(a.w2 + (size_t)tid * a.ld2 + a4);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(a.w2 + (size_t)(tid + 256) * a.ld2 + a4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { w2s[a4 + q][tid] = x0[q]; w2s[a4 + q][tid + 256] = x1[q]; }
    }
    f32x16 accw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) accw[t][r] = 0.f;
    float db0 = 0.f, db1 = 0.f;
    const int r8 = tid >> 3, c4 = (tid & 7) * 4;              // the staging and epilogue element of this thread: row r8, floats c4 ... + 3
    const int j4 = 4 * (tid & 127), rh = tid >> 7;            // dh1: columns j4 ... + 3 of rows rh + 2 e

    for (int rt = 0; rt < a.row_tiles; ++rt) {
        const int m0 = rt * 32;
        {   // stage dq (rows >= B: zero) and the a3 tile (rows >= B: row B - 1, never stored)
            const int m = m0 + r8, mc = min(m, a.B - 1);
            f32x4 d = *reinterpret_cast<const f32x4*>(a.dq + (size_t)mc * a.ld2 + c4);
            const f32x4 x = *reinterpret_cast<const f32x4*>(a.a3 + (size_t)mc * 3136 + kt * 32 + c4);
            if (m >= a.B) d = f32x4{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(&dqs[r8][c4]) = d;
#pragma unroll
            for (int q = 0; q < 4; ++q) a3s[r8][c4 + q] = x[q];
        }
        __syncthreads();
        // ---- dh1 of the row tile, two halves of eight rows per thread
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 hm[8], acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int r = rh + 2 * (8 * half + e);
                hm[e] = *reinterpret_cast<const f32x4*>(a.h1 + (size_t)min(m0 + r, a.B - 1) * 512 + j4);
                acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            for (int aa = 0; aa < a.A; ++aa) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(&w2s[aa][j4]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = dqs[rh + 2 * (8 * half + e)][aa];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[e][q] = __builtin_fmaf(d, w[q], acc[e][q]);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (!(hm[e][q] > 0.f)) acc[e][q] = 0.f;
                *reinterpret_cast<f32x4*>(&dhs[rh + 2 * (8 * half + e)][j4]) = acc[e];
            }
        }
        __syncthreads();
        if (kt == rt) {                                       // this row tile's dh1 rows -> dy[0]
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = rh + 2 * e;
                if (m0 + r < a.B) *reinterpret_cast<f32x4*>(a.dh1 + (size_t)(m0 + r) * 512 + j4) = *reinterpret_cast<const f32x4*>(&dhs[r][j4]);
            }
        }
        if (kt == CHB_KT - 1) {                               // db1: columns 2 tid, 2 tid + 1 (rows >= B are zero)
            float p0[4] = {0.f, 0.f, 0.f, 0.f}, p1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int r = 0; r < 8; ++r) { p0[k] += dhs[8 * k + r][2 * tid]; p1[k] += dhs[8 * k + r][2 * tid + 1]; }
            db0 += (p0[0] + p0[1]) + (p0[2] + p0[3]);
            db1 += (p1[0] + p1[1]) + (p1[2] + p1[3]);
        }
        // ---- (a) dW1: four column tiles per wave, two batch rows per MFMA
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int b = 2 * g + h;
            const float av = a3s[b][i];
#pragma unroll
            for (int t = 0; t < 4; ++t) accw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, dhs[b][(4 * wave + t) * 32 + i], accw[t], 0, 0, 0);
        }
        // ---- (b) dy3: dense_small_tile<true> at kred = 512, A rows from LDS, B operands from registers
        {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float* hrow = dhs[i] + 128 * wave + 4 * h;
#pragma unroll
            for (int c = 0; c < 8; ++c)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f32x4 av = *reinterpret_cast<const f32x4*>(hrow + 16 * c + 8 * u);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bw[c * 2 + u][q], acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) red[wave][(r & 3) + 8 * (r >> 2) + 4 * h][i] = acc[r];
        }
        __syncthreads();
        if (m0 + r8 < a.B) {
            f32x4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[q] = dense_small_sum(red, r8, c4 + q); if (!(a3s[r8][c4 + q] > 0.f)) v[q] = 0.f; }
            *reinterpret_cast<f32x4*>(a.dy3 + (size_t)(m0 + r8) * 3136 + kt * 32 + c4) = v;
        }
        __syncthreads();                                      // dqs, a3s, dhs and red are free for the next row tile
    }
    // ---- l1's chunk-0 partial: rows 32 kt ... + 31 from the accumulators, the bias row from workgroup CHB_KT - 1
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            a.part1[(size_t)(kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 512 + (4 * wave + t) * 32 + i] = accw[t][r];
    if (kt == CHB_KT - 1) { a.part1[(size_t)3136 * 512 + 2 * tid] = db0; a.part1[(size_t)3136 * 512 + 2 * tid + 1] = db1; }
}

hipError_t launch_cdqn_head_bwd(hipStream_t st, const CdqnHeadBwdArgs& a)
{
    return step_launch(st, false, k_cdqn_head_bwd, dim3((unsigned)(CHB_KT + 16 * (a.ld2 / 32))), dim3(256), a);
}

}  // namespace bdr
#endif  // BDR_CDQN_HEAD_BWD_KERNELS
