// Policy::sample of the candle DQN's AtariCnn Q-network on a handful of frame stacks (dqn/base.rs:202-230 is called once per
// environment step): BDR_ACT_PATH_IMAGE, two launches for n <= CAI_MAX_ROWS rows instead of the update's six batch-tiled ones.
//
//   k_cnn_act_trunk   one workgroup of four waves per observation row (grid = n): conv1, conv2 and conv3 of ONE image with every
//                     activation in LDS; the output a3 goes to feat [n][3136] in (h, w, c) order, l1's internal input layout.
//   k_cnn_act_trunk_b3  the trunk of BDR_ARITH_BF16X3_6 agents: conv2 / conv3 on the bf16 matrix cores with split operands (its own
//                     header comment, below); same grid, same feat, same head.
//   k_cnn_act_head    l1 (3136 -> 512, ReLU) cut as act_small.hpp cuts it - 16 column tiles x CAI_L1_KS k-slices, one partial
//                     32 x 32 tile per workgroup (dense_small_tile), a counter per column tile, the last arriver adds the partials in
//                     slice order - and, in the workgroup that completes the last column tile, l2 and dqn_q_argmax into the
//                     buffers k_cdqn_act writes (samp, samp_idx).
//   k_cnn_act_trunk_group, k_cnn_act_head_group   the same two launches for the selected members of a candle DQN CNN group, the
//                     member as a grid dimension (their own header comment, below; the host half: candle_dqn_cnn_group.hpp).
// No workgroup waits for another one: a counter is taken once, behind the workgroup's own stores (dense.hpp last_workgroup: agent-scope
// stores, s_waitcnt, barrier, agent-scope fetch-add), and whoever takes the last ticket goes on; the grid need not be co-resident.
//
// Arithmetic.  conv1 under conv1_bf16_img.hpp's operand rule: u8 pixels are exact in bf16, an f32 weight is split exactly into three
// bf16 terms, the products are exact, the MFMA accumulates in f32 (planes lo, mid, hi per k-step), 1/255 once in the epilogue, then
// bias and ReLU.  conv2, conv3, l1, l2: f32 x f32 on v_mfma_f32_32x32x2_f32, exact products (BDR_ARITH_F32_EXACT).  The ORDER of the
// additions differs from the batch forward (k-quarters and slices here, k-tiles there): Q agrees with the layer path to rounding, not
// bit for bit.
//
// The trunk's work split (lane = (i, h), i = lane & 31, h = lane >> 5; an MFMA tile is 32 x 32, lane (i, h) holds column i, rows
// (r & 3) + 8 (r >> 2) + 4 h of its 16 accumulators r):
//   conv1  400 positions x 32 channels, K = 64 n_stack.  Rows of the MFMA = channels, columns = 32 positions (a "unit"): 13 units,
//          wave w takes units w, w + 4, w + 8 (and 12: wave 0) and keeps their accumulators while the k-steps go by ONCE, so a
//          weight fragment is fetched and split once per wave.  Weights of a whole channel (4 k-steps) are in flight one channel ahead.
//   conv2  81 x 64, K = 512 = (kh, kw, c): 3 x 2 tiles do not divide over four waves, so the REDUCTION is split: wave w owns kernel
//          row kh = w (k in [128 w, 128 w + 128)) of all six tiles; the quarters meet in LDS - wave 0 writes a2 itself, waves 1 ... 3 the
//          reduction area - and every element is summed as ((q0 + q1) + q2) + q3, then bias and ReLU.
//   conv3  49 x 64, K = 576: 2 x 2 tiles, one per wave; one tap (64 k) of weights in flight ahead of the tap being multiplied.
//   A operands are gathered from LDS patches (16-byte reads), B operands (weights) go from L2 straight into registers: 312 KB of conv
//   weights is not staged.  Every weight address is a function of the thread index and the loop counters alone; the first weights of
//   conv1, conv2 AND conv3 and the biases of conv1 and conv3 are requested before the frames are staged.
//   Rows >= 400 / 81 / 49 of a ragged tile read the layer's last valid row (index clamped) and are not stored.
//
// LDS of the trunk, floats unless said otherwise (static, 141 840 bytes of the CU's 160 KB):
//   s_u   [15 552]        first the frames as u8 [n_stack][84][84] (7 056 n_stack <= 56 448 bytes), overlaid once conv1 is done
//                         (barrier) by conv2's reduction area red [3][81][64] (62 208 bytes)
//   s_a1  [400][36]       conv1's output; rows padded by 4 floats (57 600 bytes)
//   s_a2  [81][68]        conv2's output, padded alike (22 032 bytes)
// Index bounds.
//   frames: staged as dwords (or 16-byte vectors) t < 1 764 n_stack; conv1 reads two dwords at byte c 7056 + (4 oh + kh) 84 + 4 ow,
//           c < n_stack, oh, ow <= 19 (position index clamped to 399), kh <= 7: row <= 83, last byte column 4 * 19 + 7 = 83.
//   W1:     row 64 c + 16 sl + 8 h + j < 64 n_stack, column i < 32.   s_a1 writes: position m < 400, channels 8 q + 4 h + e < 32.
//   conv2:  position m <= 80 (clamped), a1 row (2 oh + w) 20 + 2 ow + kw <= 19 * 20 + 19 = 399, channels (s & 3) 8 + 4 h + e < 32;
//           W2 row 128 w + 8 s + 4 h + q < 512, column 32 nt + i < 64; red / s_a2 writes at m < 81 only, column < 64.
//   conv3:  position m <= 48 (clamped), a2 row (oh + kh) 9 + ow + kw <= 8 * 9 + 8 = 80, channels 8 s + 4 h + e < 64;
//           W3 row 64 tap + 8 s + 4 h + q < 576; feat writes at m < 49: row blockIdx.x < n, element m 64 + column < 3 136.
// The head: feat rows min(i, n - 1) < n, k < 3 136; W1 (l1) rows < 3 136, columns < 512; part [KS][32][512] at rows m < n, then
// h1 [32][512]; counters [17]; l2: hs rows < 32 (rows >= n hold a copy of row n - 1), W2 rows < 512, columns 32 t + i < ld2 for the
// tiles t with 32 t < A; q at m < n, column < A; idx at m < n.
// The kernels are compiled in a translation unit of their own (cnn_act_img.hip defines BDR_CNN_ACT_IMG_KERNELS; build.py compiles it
// with the packed-f32 instructions switched off); candle_dqn.hip sees the argument structs and the two launchers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace bdr {

constexpr int CAI_MAX_ROWS = 32;          // rows per call served by this path: one 32-row tile of l1
constexpr int CAI_A1_LD = 36, CAI_A2_LD = 68;
constexpr int CAI_RED = 81 * 64;          // floats of one k-quarter of conv2
constexpr int CAI_L1_KS = 7;              // k-slices of l1: 448 k each (act_small.hpp: 49 slices of one round trip each were slower)
constexpr size_t CAI_PART_FLOATS = (size_t)(CAI_L1_KS + 1) * 32 * 512;   // the partial tiles, then h1 [32][512]
constexpr int CAI_COUNTERS = 17;          // one per column tile of l1, one for the layer

struct CnnActTrunkArgs {
    const uint8_t* rows; size_t row_stride;   // n frame stacks [n_stack][84][84] u8, row_stride bytes apart (a multiple of 4)
    int ns, vec16;                            // vec16: base and stride are multiples of 16 bytes
    const float *w1, *b1, *w2, *b2, *w3, *b3; // conv_layout.hpp's internal layouts
    float* feat;                              // [n][3136]
};

struct CnnActHeadArgs {
    const float* feat;                 // [n][3136]
    const float *w1, *b1;              // l1: [3136][512], [512]
    const float *w2, *b2; int ld2;     // l2: [512][ld2], [A]
    float* part;                       // CAI_PART_FLOATS: [CAI_L1_KS][32][512] partial tiles, then h1 [32][512]
    unsigned* counters;                // [CAI_COUNTERS], zero between launches
    int n, A;
    float* q; long long* idx;          // [n][A], [n]
};

// k_cnn_act_trunk_b3 (BDR_ARITH_BF16X3_6): W2 / W3 come as the parameter set's bf16 planes (fwd_c23_b3.hpp: CPL_W2, CPL_W3)
struct CnnActTrunkB3Args {
    const uint8_t* rows; size_t row_stride;
    int ns, vec16;
    const float *w1, *b1;
    const uint16_t* pl2; const float* b2;     // [3][16][64][32]
    const uint16_t* pl3; const float* b3;     // [3][18][64][32]
    float* feat;                              // [n][3136]
    float *keep_a1, *keep_a2;                 // null, or [n][20][20][32] and [n][9][9][64]: the probes' copies of a1 and a2
};

hipError_t launch_cnn_act_trunk(hipStream_t st, int n, const CnnActTrunkArgs& a);   // grid n
hipError_t launch_cnn_act_trunk_b3(hipStream_t st, int n, const CnnActTrunkB3Args& a);   // grid n
hipError_t launch_cnn_act_head(hipStream_t st, const CnnActHeadArgs& a);            // grid (16, CAI_L1_KS)

// ---- the group entries (candle_dqn_cnn_group.hpp): Policy::sample of the selected members of a group, the member = sel[blockIdx.y]
// (trunk) / sel[blockIdx.z] (head).  `trunk` and `head` are device arrays [P] of the members' STATIC words, read in place through the
// constant address space: the member is uniform, so its fields stay scalar loads.  A static trunk entry holds the weights, ns,
// row_stride = 7056 ns, vec16 = 1 and feat = the group's feature area [n_sel][32][3136] (rows: null - the call's); a static head entry
// the weights, ld2, A, feat = the same area, the member's OWN part / counters and q = the member's own device rows [32][A] (n, idx:
// unused - the call's).  `calls` [P] and `sel` [n_sel] are this call's, in pinned device-mapped memory.
struct CnnActGroupCall {
    const uint8_t* rows;   // the member's n staged frame stacks, 16-byte aligned, 7056 ns bytes apart
    float* res;            // the member's result block in pinned memory: Q [n][A] floats, then the n first-maximum indices as int32
};
struct CnnActGroupDone { unsigned* ticket; unsigned* seq_host; unsigned seq; };   // the group's ticket (group_done.hpp) and this launch's number
hipError_t launch_cnn_act_trunk_group(hipStream_t st, int n, unsigned n_sel, const CnnActTrunkArgs* trunk, const CnnActGroupCall* calls,
                                      const unsigned* sel);   // grid (n, n_sel)
hipError_t launch_cnn_act_head_group(hipStream_t st, int n, unsigned n_sel, const CnnActHeadArgs* head, const CnnActGroupCall* calls,
                                     const unsigned* sel, const CnnActGroupDone& done);   // grid (16, CAI_L1_KS, n_sel)

}  // namespace bdr

#ifdef BDR_CNN_ACT_IMG_KERNELS
#include "conv1_bf16.hpp"
#include "dense.hpp"
#include "dense_act.hpp"
#include "fwd_c23_b3.hpp"   // k_cnn_act_trunk_b3: the plane layouts (cpl_index, c23_a1_off, c23_a2_off) and split3_f32x4
#include "group_done.hpp"   // the group entries end with the group's ticket

namespace bdr {

// n elements src -> dst, eight loads of a thread in flight at a time (index clamped for the load, predicated for the store)
template <class V>
__device__ __forceinline__ void cai_stage(const V* __restrict__ src, V* dst, int n, int tid)
{
    for (int t0 = 0; t0 < n; t0 += 256 * 8) {
        V v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int t = t0 + 256 * k + tid; v[k] = src[t < n ? t : n - 1]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int t = t0 + 256 * k + tid; if (t < n) dst[t] = v[k]; }
    }
}

static __global__ __launch_bounds__(256) void k_cnn_act_trunk(CnnActTrunkArgs a)
{
#include "cnn_act_trunk_body_inc.hpp"
}


// ---- k_cnn_act_trunk_b3 -----------------------------------------------------------------------------------------------------------
// The trunk of BDR_ARITH_BF16X3_6 agents: conv2 and conv3 on v_mfma_f32_32x32x16_bf16 with both operands split into three bf16 terms
// (igemm_b3.hpp split3_rn / split3_f32x4) and six of the nine partial products kept.  One workgroup of four waves per frame stack, as
// k_cnn_act_trunk; the data path is its own:
//   conv1  k_cnn_act_trunk's (same units, same operand rule, same sums).  Its epilogue splits every run of four channels ONCE and
//          leaves a1 in LDS as three bf16 planes in k_fwd_c23_b3's layout: four parity blocks (ih & 1, iw & 1) of [10][10] pixels of
//          64 bytes, the four 16-byte chunks of pixel P at chunk ^ ((P >> 2) & 3) (c23_a1_off), so that the 16 lanes of a
//          ds_read_b128 group read 16 different 16-byte slots.
//   conv2  rows of the MFMA = 32 output channels, columns = 32 positions, column v = 10 oh + ow (ow = 9 is a hole: 89 columns in three
//          tiles).  Six products per 16 k cost 192 matrix cycles where the FP32 MFMA costs 512, so the six tiles need NO k split:
//          the waves take 2 / 2 / 1 / 1 tiles - wave 0 and wave 1 position tile 0 / 1 with both channel tiles, waves 2 and 3 position
//          tile 2 with channel tile 0 / 1 - and the reduction area of the exact trunk is gone.  The epilogue (bias, ReLU) splits a2
//          once into three planes [84 pixels][64] (chunk ^ ((P >> 1) & 7): c23_a2_off) that OVERLAY the frames, dead since conv1.
//   conv3  2 x 2 tiles, one per wave: column v = 9 oh + ow (ow = 7, 8 and oh = 7 are holes: 63 columns in two tiles); a3 -> feat.
//   A fragments (activations) are 16-byte LDS reads of the planes; B fragments (weights) go from the pre-split planes in L2 straight
//   into registers as 16-byte pieces, in chunks (a k-tile of 32 = two MFMA steps) held in a ring of four (conv2) / three (conv3):
//   a chunk's slot is refilled as soon as it has been multiplied, so three / two chunks are in flight ahead of the one in use (one
//   chunk ahead left every chunk's ~0.3 us of matrix work waiting for a load from L2: 55 us against 41 us for the trunk at n = 1).
//   Chunk 0 of conv2 AND of conv3, conv1's first channel and all three biases are requested before the frames are staged.
// Summation order: every output element of conv2 / conv3 is ONE f32 accumulator that sees k ascending in steps of 16 in (kh, kw, c)
// order, lane half h holding k = 8 h ... 8 h + 7 of a step, and per step the products (activation term, weight term) =
// (2,0) (0,2) (1,1) (1,0) (0,1) (0,0) - ORD9[3..8] of k_igemm_b3, smallest first.  That is k_fwd_c23_b3's order: a2 is what the
// layer path computes from the same a1, bit for bit, and a3 from the same a2.  (a1 itself differs from the layer path's in the
// order of conv1's sums, as in the exact trunk.)
// Registers: 254 VGPRs + 112 AGPRs, no scratch.  The 2-tile waves' conv2 ring alone is 4 chunks x 48 = 192 registers and the
// allocator stops at 256 VGPRs, so there is no headroom: if a compiler change makes this kernel spill, a ring of three chunks for
// conv2 (16 k-tiles: peel the last one) is the fallback, at some of the latency cover.
// Hole columns read real or padding pixels (never written: any bit pattern) and are never stored; an MFMA column depends on its own
// column of the operand only.
// LDS (static, 139 392 bytes of the CU's 160 KB, whatever n_stack <= 8 is):
//   s_fr  [56 448 bytes]  the frames as u8 [n_stack][84][84]; behind conv1's barrier a2's planes [3][84][64] bf16 (32 256 bytes)
//   s_p1  [3][432][32]    a1's planes, bf16 (82 944 bytes)
// Index bounds.
//   frames, W1, conv1's units: k_cnn_act_trunk's.   s_p1 writes: position m < 400 = (ih, iw), pixel P = ((ih & 1) 2 + (iw & 1)) 108 +
//           10 (ih >> 1) + (iw >> 1) <= 3 * 108 + 99, chunk q < 4, half h: u16 offset < 432 * 32 per plane.
//   conv2:  column v = 32 pt + i <= 95, pixel v + 10 (kh >> 1) + (kw >> 1) <= 95 + 11 = 106 < 108 of block (kh & 1, kw & 1), chunk
//           2 s + h < 4;  plane index cpl_index(32 kt + 16 s + 8 h, 32 ct + i) + 7 <= (15 * 64 + 63) 32 + 31 < 64 * 512;
//           s_p2 writes at oh, ow < 9 only: pixel m <= 80, chunk 4 ct + q < 8;  keep_a2 row blockIdx.x < n, element m 64 + channel < 5 184.
//   conv3:  column v = 32 pt + i <= 63, pixel v + 9 kh + kw <= 63 + 20 = 83 < 84, chunk 4 (kt & 1) + 2 s + h < 8;
//           plane index <= (17 * 64 + 63) 32 + 31 < 64 * 576;  feat writes at oh, ow < 7: row blockIdx.x < n, element (7 oh + ow) 64 +
//           32 ct + 8 q + 4 h + 3 < 3 136.   keep_a1 row blockIdx.x < n, element m 32 + channel < 12 800.
constexpr int CAB_FRAME_BYTES = 7056 * C1_MAX_STACK;
static_assert(3 * C23_PL_A2 * 2 <= CAB_FRAME_BYTES, "a2's planes overlay the frames");
static_assert(CAB_FRAME_BYTES + 3 * C23_PL_A1 * 2 <= 160 * 1024, "one workgroup per CU");

static __global__ __launch_bounds__(256) void k_cnn_act_trunk_b3(CnnActTrunkB3Args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_fr[CAB_FRAME_BYTES / 4];
    __shared__ __attribute__((aligned(16))) uint16_t s_p1[3 * C23_PL_A1];
    uint16_t* const s_p2 = reinterpret_cast<uint16_t*>(s_fr);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    constexpr int ORD[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};   // (activation term, weight term)
    // conv2: position tile pt2 and channel tiles ct2(0 ... nt2 - 1) of this wave; conv3: tile (pt3, ct3)
    const int pt2 = min(wave, 2), nt2 = wave < 2 ? 2 : 1, ct2_0 = wave < 2 ? 0 : wave - 2;
    const int pt3 = wave >> 1, ct3 = wave & 1;

    // ---- every first operand, requested before anything is waited for
    auto load_w1 = [&](int c, float (&w)[4][8]) __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < 4; ++sl)
#pragma unroll
            for (int j = 0; j < 8; ++j) w[sl][j] = a.w1[(size_t)(64 * c + 16 * sl + 8 * h + j) * 32 + i];
    };
    // chunk kt of conv2: the fragments of its two k-steps, this wave's channel tiles, three planes: 8 bf16 at cpl_index(32 kt + 16 s + 8 h, n)
    auto load_w2 = [&](int kt, bf16x8_t (&w)[2][2][3]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
                if (tn < nt2)   // wave-uniform
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
                        w[s][tn][pl] = *reinterpret_cast<const bf16x8_t*>(a.pl2 + (size_t)pl * (64 * 512) + cpl_index(32 * kt + 16 * s + 8 * h, 32 * (ct2_0 + tn) + i));
    };
    auto load_w3 = [&](int kt, bf16x8_t (&w)[2][3]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                w[s][pl] = *reinterpret_cast<const bf16x8_t*>(a.pl3 + (size_t)pl * (64 * 576) + cpl_index(32 * kt + 16 * s + 8 * h, 32 * ct3 + i));
    };
    float w1n[4][8];
    bf16x8_t w2b[4][2][2][3], w3b[3][2][3];   // rings of four / three chunks: a chunk is requested three / two chunks before it is multiplied
    load_w1(0, w1n);
    f32x4 bq1[4], bq2[2][4], bq3[4];   // the bias of this lane's channel runs [8 q + 4 h, + 4) of each of its tiles
#pragma unroll
    for (int q = 0; q < 4; ++q) bq1[q] = *reinterpret_cast<const f32x4*>(a.b1 + 8 * q + 4 * h);
    load_w2(0, w2b[0]);
    load_w3(0, w3b[0]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
            if (tn < nt2) bq2[tn][q] = *reinterpret_cast<const f32x4*>(a.b2 + 32 * (ct2_0 + tn) + 8 * q + 4 * h);
        bq3[q] = *reinterpret_cast<const f32x4*>(a.b3 + 32 * ct3 + 8 * q + 4 * h);
    }

    // ---- the frame stack -> LDS, as it is (u8)
    {
        const uint8_t* src = a.rows + (size_t)blockIdx.x * a.row_stride;
        if (a.vec16) cai_stage(reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(s_fr), a.ns * 441, tid);
        else cai_stage(reinterpret_cast<const uint32_t*>(src), s_fr, a.ns * 1764, tid);
    }
    __syncthreads();

    // ---- conv1 (k_cnn_act_trunk's k loop); the epilogue leaves a1 split in s_p1
    {
        const int nu = wave == 0 ? 4 : 3;
        const uint8_t* frb = reinterpret_cast<const uint8_t*>(s_fr);
        int poff[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = min((wave + 4 * t) * 32 + i, 399), oh = m / 20, ow = m - oh * 20;
            poff[t] = (oh * 4 + h) * 84 + ow * 4;
        }
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        for (int c = 0; c < a.ns; ++c) {
            float wc[4][8];
#pragma unroll
            for (int sl = 0; sl < 4; ++sl)
#pragma unroll
                for (int j = 0; j < 8; ++j) wc[sl][j] = w1n[sl][j];
            if (c + 1 < a.ns) load_w1(c + 1, w1n);
#pragma unroll
            for (int sl = 0; sl < 4; ++sl) {
                uint32_t hi[8], mid[8], lo[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    hi[j] = __float_as_uint(wc[sl][j]) & 0xffff0000u;
                    const float r1 = wc[sl][j] - __uint_as_float(hi[j]);    // exact
                    mid[j] = __float_as_uint(r1) & 0xffff0000u;
                    const float r2 = r1 - __uint_as_float(mid[j]);          // exact, <= 8 significant bits
                    lo[j] = __float_as_uint(r2) & 0xffff0000u;
                }
                bf16x8 wp[3];
                wp[0] = __builtin_bit_cast(bf16x8, uint4{(hi[0] >> 16) | hi[1], (hi[2] >> 16) | hi[3], (hi[4] >> 16) | hi[5], (hi[6] >> 16) | hi[7]});
                wp[1] = __builtin_bit_cast(bf16x8, uint4{(mid[0] >> 16) | mid[1], (mid[2] >> 16) | mid[3], (mid[4] >> 16) | mid[5], (mid[6] >> 16) | mid[7]});
                wp[2] = __builtin_bit_cast(bf16x8, uint4{(lo[0] >> 16) | lo[1], (lo[2] >> 16) | lo[3], (lo[4] >> 16) | lo[5], (lo[6] >> 16) | lo[7]});
                const int so = c * 7056 + (2 * sl) * 84;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t < nu) {   // wave-uniform
                        const uint32_t* px = reinterpret_cast<const uint32_t*>(frb + poff[t] + so);
                        const bf16x8 fa = u8x8_to_bf16(px[0], px[1]);
#pragma unroll
                        for (int pl = 2; pl >= 0; --pl) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wp[pl], fa, acc[t], 0, 0, 0);   // small terms first
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = (wave + 4 * t) * 32 + i;
            if (t < nu && m < 400) {
                const int ih = m / 20, iw = m - ih * 20;
                const int P = ((ih & 1) * 2 + (iw & 1)) * C23_A1_BLK + (ih >> 1) * 10 + (iw >> 1);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float x = acc[t][4 * q + e] * (1.0f / 255.0f) + bq1[q][e]; v[e] = x > 0.f ? x : 0.f; }
                    u32x2_t sp[3];
                    split3_f32x4(v, sp);
                    const int o = c23_a1_off(P, q) + 4 * h;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x2_t*>(&s_p1[pl * C23_PL_A1 + o]) = sp[pl];
                    if (a.keep_a1) *reinterpret_cast<f32x4*>(a.keep_a1 + ((size_t)blockIdx.x * 400 + m) * 32 + 8 * q + 4 * h) = v;   // workgroup-uniform
                }
            }
        }
    }
    __syncthreads();   // a1's planes are whole; nobody reads the frames any more: a2's planes may overlay them

    // ---- conv2: position tile pt2, channel tiles ct2_0 ... of this wave, all 16 k-tiles (taps) in order
    {
        const int v = pt2 * 32 + i;
        f32x16 acc[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tn][r] = 0.f;
#pragma unroll
        for (int u = 1; u < 4; ++u) load_w2(u, w2b[u]);
        for (int kt0 = 0; kt0 < 16; kt0 += 4) {   // kernel row kh = kt0 >> 2; ring slot u = kw
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kh = kt0 >> 2, kw = u;
                const int P = ((kh & 1) * 2 + (kw & 1)) * C23_A1_BLK + v + 10 * (kh >> 1) + (kw >> 1);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bf16x8_t fx[3];
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) fx[pl] = *reinterpret_cast<const bf16x8_t*>(&s_p1[pl * C23_PL_A1 + c23_a1_off(P, 2 * s + h)]);
#pragma unroll
                    for (int t = 0; t < 6; ++t)
#pragma unroll
                        for (int tn = 0; tn < 2; ++tn)
                            if (tn < nt2) acc[tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2b[u][s][tn][ORD[t][1]], fx[ORD[t][0]], acc[tn], 0, 0, 0);
                }
                if (kt0 + 4 < 16) load_w2(kt0 + 4 + u, w2b[u]);   // (kt0 + 4 + u <= 15)
            }
        }
#pragma unroll
        for (int u = 1; u < 3; ++u) load_w3(u, w3b[u]);   // in flight across the epilogue and the barrier
        const int oh = v / 10, ow = v - 10 * oh;
        if (oh < 9 && ow < 9) {
            const int m = oh * 9 + ow;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
                if (tn < nt2) {
                    const int ct = ct2_0 + tn;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4 y;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const float t = acc[tn][4 * q + e] + bq2[tn][q][e]; y[e] = t > 0.f ? t : 0.f; }
                        u32x2_t sp[3];
                        split3_f32x4(y, sp);
                        const int o = c23_a2_off(m, 4 * ct + q) + 4 * h;
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x2_t*>(&s_p2[pl * C23_PL_A2 + o]) = sp[pl];
                        if (a.keep_a2) *reinterpret_cast<f32x4*>(a.keep_a2 + ((size_t)blockIdx.x * 81 + m) * 64 + 32 * ct + 8 * q + 4 * h) = y;
                    }
                }
        }
    }
    __syncthreads();   // a2's planes are whole

    // ---- conv3: tile (pt3, ct3), all 18 k-tiles (half taps) in order
    {
        const int v = pt3 * 32 + i;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int kt0 = 0; kt0 < 18; kt0 += 3) {
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int kt = kt0 + u, tap = kt >> 1, kh = tap / 3, kw = tap - 3 * kh, P = v + 9 * kh + kw;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bf16x8_t fx[3];
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) fx[pl] = *reinterpret_cast<const bf16x8_t*>(&s_p2[pl * C23_PL_A2 + c23_a2_off(P, (kt & 1) * 4 + 2 * s + h)]);
#pragma unroll
                    for (int t = 0; t < 6; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3b[u][s][ORD[t][1]], fx[ORD[t][0]], acc, 0, 0, 0);
                }
                if (kt0 + 3 < 18) load_w3(kt + 3, w3b[u]);   // (kt + 3 <= 17)
            }
        }
        const int oh = v / 9, ow = v - 9 * oh;
        if (oh < 7 && ow < 7) {
            float* out = a.feat + (size_t)blockIdx.x * 3136 + (oh * 7 + ow) * 64 + 32 * ct3 + 4 * h;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 y;
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float t = acc[4 * q + e] + bq3[q][e]; y[e] = t > 0.f ? t : 0.f; }
                *reinterpret_cast<f32x4*>(out + 8 * q) = y;
            }
        }
    }
}

// grid (16, CAI_L1_KS)
static __global__ __launch_bounds__(256) void k_cnn_act_head(CnnActHeadArgs a)
{
    __shared__ float red[4][32][33];
    __shared__ __attribute__((aligned(16))) float hs[32][516];
    __shared__ unsigned s_last;
    constexpr int KSL = 3136 / CAI_L1_KS;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = blockIdx.x, ks = blockIdx.y, n0 = nt * 32, k0 = ks * KSL;
    const float* arow = a.feat + (size_t)min(lane & 31, a.n - 1) * 3136 + k0;   // rows >= n alias the last row (never stored)
    const int r = tid >> 3, c4 = (tid & 7) * 4, col = n0 + c4;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b1 + col);   // the epilogue's operand, requested beside the tile operands
    dense_small_tile<false>([&](int k) { return *reinterpret_cast<const f32x4*>(arow + k); }, a.w1 + (size_t)k0 * 512, 512, n0, KSL, wave, lane, red);
    __syncthreads();
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = dense_small_sum(red, r, c4 + q);
    if (r < a.n) {
        float* p = a.part + ((size_t)ks * 32 + r) * 512 + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) st_agent(p + q, v[q]);
    }
    if (!last_workgroup(a.counters + nt, (unsigned)CAI_L1_KS, &s_last)) return;
    // the column tile's partials in slice order whoever arrives last (act_small.hpp: 16-byte loads served by the coherent level, all
    // in flight before the one wait)
    float* h1 = a.part + (size_t)CAI_L1_KS * 32 * 512;
    if (r < a.n) {
        const float* p0 = a.part + (size_t)r * 512 + col;
        f32x4 t[CAI_L1_KS];
#pragma unroll
        for (int e = 0; e < CAI_L1_KS; ++e) {
            const float* ps = p0 + (size_t)e * 32 * 512;
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(t[e]) : "v"(ps) : "memory");
        }
        static_assert(CAI_L1_KS == 7, "the wait below names seven destinations");
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]) :: "memory");
        v = t[0];
#pragma unroll
        for (int e = 1; e < CAI_L1_KS; ++e) v += t[e];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = v[q] + bv[q];
            st_agent(h1 + (size_t)r * 512 + col + q, x > 0.f ? x : 0.f);   // read by the workgroup below, possibly on another XCD
        }
    }
    if (!last_workgroup(a.counters + 16, 16u, &s_last)) return;

    // ---- l2 and the first maximum, by the workgroup that completed l1's last column tile: h1 -> LDS (rows >= n: a copy of row n - 1)
    for (int e0 = 0; e0 < 16; e0 += 8) {
        f32x4 t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int x = tid + 256 * (e0 + e);   // 16-byte vector x of hs: row x >> 7, floats 4 (x & 127) ...
            const float* ps = h1 + (size_t)min(x >> 7, a.n - 1) * 512 + 4 * (x & 127);
            asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(t[e]) : "v"(ps) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]) :: "memory");
#pragma unroll
        for (int e = 0; e < 8; ++e) { const int x = tid + 256 * (e0 + e); *reinterpret_cast<f32x4*>(&hs[x >> 7][4 * (x & 127)]) = t[e]; }
    }
    __syncthreads();
    const float* hrow = hs[lane & 31];
    for (int t0 = 0; t0 < a.A; t0 += 32) {
        dense_small_tile<false>([&](int k) { return *reinterpret_cast<const f32x4*>(hrow + k); }, a.w2, a.ld2, t0, 512, wave, lane, red);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = t0 + c4 + q;
            if (r < a.n && j < a.A) a.q[(size_t)r * a.A + j] = dense_small_sum(red, r, c4 + q) + a.b2[j];
        }
        __syncthreads();   // red is free again; the Q stores of this workgroup are visible to it
    }
    if (tid < a.n) a.idx[tid] = dqn_q_argmax(a.q + (size_t)tid * a.A, a.A);
}

// ---- the group entries ---------------------------------------------------------------------------------------------------------------
// k_cnn_act_trunk_group   grid (n, n_sel): one workgroup of four waves per (frame stack, selected member) runs k_cnn_act_trunk's body -
//   the same text (cnn_act_trunk_body_inc.hpp): conv1's units per wave on the bf16 MFMA with split weights, conv2's k-quarters meeting in
//   LDS as ((q0 + q1) + q2) + q3, conv3 one tile per wave, weights from L2 straight into registers one step ahead - on a CnnActTrunkArgs
//   gathered in registers from the member's static entry (scalar loads), the member's rows of this call and the block of 32 feature
//   rows of the SELECTION index y.  Same sums, same bits as the member's own k_cnn_act_trunk.
// k_cnn_act_head_group    grid (16 column tiles, CAI_L1_KS k-slices, n_sel): k_cnn_act_head's tiles and sums per member - one partial
//   32 x 32 tile per workgroup (dense_small_tile), the member's own counter per column tile, the last arriver adds the partials in
//   slice order, and the workgroup that completes the member's last column tile runs l2 and dqn_q_argmax - with a body of its own,
//   because every workgroup has to reach the group's ticket: the two early returns of the standalone head are nested conditions here.
//   Q goes to the member's device rows q (the argmax reads them back, as the standalone head reads samp) AND to the member's block of
//   the pinned result area; the indices go to the block only.  Every thread fences its result stores at system scope before its
//   workgroup counts on the ticket (candle_act_group.hpp's rule); the last workgroup of the launch publishes the launch number.
//   A member's counters are zero between launches: whoever takes the last ticket of a counter re-arms it (dense.hpp ticket_take).
// No workgroup waits for another one; the grids need not be co-resident.
// Bounds of every new index.  y (z) = blockIdx.y (.z) < gridDim.y (.z) = n_sel = the length of `sel` the host has written; member =
// sel[y] < P = the length of `trunk`, `head` and `calls` (checked by the host before anything is enqueued).  The trunk reads frame stack
// blockIdx.x < n of the member's n staged rows and writes feature row y * 32 + blockIdx.x < n_sel * 32 of feat [n_sel][32][3136]
// (n <= CAI_MAX_ROWS = 32).  The head reads feature rows y * 32 + min(i, n - 1); part, counters and q are the member's own
// (CAI_PART_FLOATS floats, CAI_COUNTERS words, 32 * A floats), indexed inside as k_cnn_act_head indexes them: part at rows r < n, h1
// likewise, counters nt < 16 and 16.  Result stores go only to rows r < n: res[r * A + j], j < A, and int32 index n * A + tid, tid < n,
// inside the member's block of n * (A + 1) floats.
static __global__ __launch_bounds__(256) void k_cnn_act_trunk_group(const BDR_CONST_AS CnnActTrunkArgs* args, const BDR_CONST_AS CnnActGroupCall* calls,
                                                                    const BDR_CONST_AS unsigned* sel)
{
    const unsigned member = sel[blockIdx.y];
    const BDR_CONST_AS CnnActTrunkArgs& e = args[member];
    const CnnActTrunkArgs a{calls[member].rows, e.row_stride, e.ns, e.vec16, e.w1, e.b1, e.w2, e.b2, e.w3, e.b3, e.feat + (size_t)blockIdx.y * (CAI_MAX_ROWS * 3136)};
#include "cnn_act_trunk_body_inc.hpp"
}

static __global__ __launch_bounds__(256) void k_cnn_act_head_group(const BDR_CONST_AS CnnActHeadArgs* args, const BDR_CONST_AS CnnActGroupCall* calls,
                                                                   const BDR_CONST_AS unsigned* sel, int n, CnnActGroupDone done)
{
    __shared__ float red[4][32][33];
    __shared__ __attribute__((aligned(16))) float hs[32][516];
    __shared__ unsigned s_last;
    constexpr int KSL = 3136 / CAI_L1_KS;
    const unsigned member = sel[blockIdx.z];
    const BDR_CONST_AS CnnActHeadArgs& a = args[member];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = blockIdx.x, ks = blockIdx.y, n0 = nt * 32, k0 = ks * KSL;
    const int A = a.A, ld2 = a.ld2;
    float* const part = a.part;
    unsigned* const counters = a.counters;
    const float* arow = a.feat + ((size_t)blockIdx.z * CAI_MAX_ROWS + min(lane & 31, n - 1)) * 3136 + k0;   // rows >= n alias the last row (never stored)
    const int r = tid >> 3, c4 = (tid & 7) * 4, col = n0 + c4;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b1 + col);
    dense_small_tile<false>([&](int k) { return *reinterpret_cast<const f32x4*>(arow + k); }, a.w1 + (size_t)k0 * 512, 512, n0, KSL, wave, lane, red);
    __syncthreads();
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = dense_small_sum(red, r, c4 + q);
    if (r < n) {
        float* p = part + ((size_t)ks * 32 + r) * 512 + col;
#pragma unroll
        for (int q = 0; q < 4; ++q) st_agent(p + q, v[q]);
    }
    if (last_workgroup(counters + nt, (unsigned)CAI_L1_KS, &s_last)) {
        // the column tile's partials in slice order whoever arrives last (k_cnn_act_head's loads and sums)
        float* h1 = part + (size_t)CAI_L1_KS * 32 * 512;
        if (r < n) {
            const float* p0 = part + (size_t)r * 512 + col;
            f32x4 t[CAI_L1_KS];
#pragma unroll
            for (int e = 0; e < CAI_L1_KS; ++e) {
                const float* ps = p0 + (size_t)e * 32 * 512;
                asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(t[e]) : "v"(ps) : "memory");
            }
            static_assert(CAI_L1_KS == 7, "the wait below names seven destinations");
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]) :: "memory");
            v = t[0];
#pragma unroll
            for (int e = 1; e < CAI_L1_KS; ++e) v += t[e];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float x = v[q] + bv[q];
                st_agent(h1 + (size_t)r * 512 + col + q, x > 0.f ? x : 0.f);   // read by the workgroup below, possibly on another XCD
            }
        }
        if (last_workgroup(counters + 16, 16u, &s_last)) {
            // ---- l2 and the first maximum, by the workgroup that completed the member's last column tile
            for (int e0 = 0; e0 < 16; e0 += 8) {
                f32x4 t[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int x = tid + 256 * (e0 + e);   // 16-byte vector x of hs: row x >> 7, floats 4 (x & 127) ...
                    const float* ps = h1 + (size_t)min(x >> 7, n - 1) * 512 + 4 * (x & 127);
                    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(t[e]) : "v"(ps) : "memory");
                }
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]) :: "memory");
#pragma unroll
                for (int e = 0; e < 8; ++e) { const int x = tid + 256 * (e0 + e); *reinterpret_cast<f32x4*>(&hs[x >> 7][4 * (x & 127)]) = t[e]; }
            }
            __syncthreads();
            const float* hrow = hs[lane & 31];
            float* const qd = a.q;                  // the member's device rows [32][A]
            float* const res = calls[member].res;   // its block of the pinned result area
            for (int t0 = 0; t0 < A; t0 += 32) {
                dense_small_tile<false>([&](int k) { return *reinterpret_cast<const f32x4*>(hrow + k); }, a.w2, ld2, t0, 512, wave, lane, red);
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = t0 + c4 + q;
                    if (r < n && j < A) {
                        const float x = dense_small_sum(red, r, c4 + q) + a.b2[j];
                        qd[(size_t)r * A + j] = x;
                        res[(size_t)r * A + j] = x;
                    }
                }
                __syncthreads();   // red is free again; the Q stores of this workgroup are visible to it
            }
            if (tid < n) reinterpret_cast<int*>(res + (size_t)n * A)[tid] = dqn_q_argmax(qd + (size_t)tid * A, A);
        }
    }
    __threadfence_system();   // this thread's result rows are in host memory before its workgroup counts
    bg_group_done(done.ticket, done.seq_host, done.seq);
}

hipError_t launch_cnn_act_trunk_group(hipStream_t st, int n, unsigned n_sel, const CnnActTrunkArgs* trunk, const CnnActGroupCall* calls, const unsigned* sel)
{
    return step_launch(st, false, k_cnn_act_trunk_group, dim3((unsigned)n, n_sel), dim3(256), (const BDR_CONST_AS CnnActTrunkArgs*)trunk,
                       (const BDR_CONST_AS CnnActGroupCall*)calls, (const BDR_CONST_AS unsigned*)sel);
}
hipError_t launch_cnn_act_head_group(hipStream_t st, int n, unsigned n_sel, const CnnActHeadArgs* head, const CnnActGroupCall* calls, const unsigned* sel,
                                     const CnnActGroupDone& done)
{
    return step_launch(st, false, k_cnn_act_head_group, dim3(16, CAI_L1_KS, n_sel), dim3(256), (const BDR_CONST_AS CnnActHeadArgs*)head,
                       (const BDR_CONST_AS CnnActGroupCall*)calls, (const BDR_CONST_AS unsigned*)sel, n, done);
}

hipError_t launch_cnn_act_trunk(hipStream_t st, int n, const CnnActTrunkArgs& a)
{
    return step_launch(st, false, k_cnn_act_trunk, dim3((unsigned)n), dim3(256), a);
}
hipError_t launch_cnn_act_trunk_b3(hipStream_t st, int n, const CnnActTrunkB3Args& a)
{
    return step_launch(st, false, k_cnn_act_trunk_b3, dim3((unsigned)n), dim3(256), a);
}
hipError_t launch_cnn_act_head(hipStream_t st, const CnnActHeadArgs& a)
{
    return step_launch(st, false, k_cnn_act_head, dim3(16, CAI_L1_KS), dim3(256), a);
}

}  // namespace bdr
#endif  // BDR_CNN_ACT_IMG_KERNELS
