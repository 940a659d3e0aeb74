// conv2 + conv3 forward of the Nature CNN on the bf16 matrix cores with split f32 operands (igemm_b3.hpp, six of the nine partial
// products): the weight planes kept beside each parameter set, the two per-layer launches (k_igemm_b3 with the FwdB3 policies), and
// the fused per-image launch k_fwd_c23_b3 that computes a2 = relu(conv2(a1)) and a3 = relu(conv3(a2)) of whole images.
//
// Why a fused form: at B = 256 each of the two layers is a 12 / 9 us launch whose matrix work is under 4 / 3 us.  The rest is launch,
// prologue and drain, paid twice, and operand delivery that repeats itself: the im2col rows of conv2 read every a1 element 4 times
// and those of conv3 every a2 element 9 times, each time as f32 from L2 and each time split into its three bf16 terms again by the
// staging threads; a2 goes to HBM and comes back in the next launch.  Here a workgroup owns ONE image of one instance:
//  * the image's a1 (400 x 32 f32) is read once with coalesced 16-byte loads, split once (split3_f32x4) and kept in LDS as three
//    bf16 planes; conv2's patch fragments are 16-byte LDS reads;
//  * conv2's epilogue (bias, ReLU: FwdP::store's expression) stores a2 to HBM as before (conv3 dW, conv3 dX's mask and the probes
//    read it) and leaves it in LDS, split once, for conv3, which runs behind one workgroup barrier;
//  * the weights stream from the pre-split planes through two LDS stages, W2's 16 k-tiles and W3's 18 as ONE sequence of 34, so that
//    conv3's first tiles are in flight while conv2 finishes.
// Bit identity with the two launches: every output element is one f32 accumulator that sees k ascending in steps of 16 in AFwd's
// k order (kh, kw, c), lane half h holding k = 8h .. 8h + 7 of a step, and per step the six products of ORD9[3..8], smallest first,
// with v_mfma_f32_32x32x16_bf16; no k split.  The operand ROLES are swapped as in conv1_bf16_img.hpp (rows = 32 output channels,
// columns = 32 positions: the same sums element by element), so that a lane ends with runs of 4 consecutive channels of one
// position: 16-byte stores to HBM and one split3_f32x4 + 8-byte LDS store per run.
//
// Which position a column of a 32-wide tile stands for is free, and chosen so that the 16 lanes of a ds_read_b128 group always read
// 16 different 16-byte slots of the 256-byte LDS row:
//  * conv2 (stride 2): a1's pixels are stored in four blocks by the parity of (ih, iw), each [10][10] pixels of 64 B (one plane), the
//    four 16-byte chunks of pixel P at chunk ^ ((P >> 2) & 3).  Column v = 10 oh + ow (ow = 9 is a hole: 89 columns in 3 tiles) reads
//    tap (kh, kw) at pixel v + 10 (kh >> 1) + (kw >> 1) of block (kh & 1, kw & 1): consecutive lanes, consecutive pixels;
//  * conv3 (stride 1): a2's pixels as [9][9] of 128 B, the eight chunks of pixel P at chunk ^ ((P >> 1) & 7).  Column v = 9 oh + ow
//    (ow = 7, 8 and oh = 7 are holes: 63 columns in 2 tiles) reads tap (kh, kw) at pixel v + 9 kh + kw.
// Hole columns read real or padding pixels and are never stored (an MFMA column depends on its own column of the operand only).
// Wave balance: conv2 is 3 position tiles x 2 channel tiles; waves 0-2 take one position tile with both channel tiles (two
// accumulators), wave 3 only stages weights - six 32 x 32 tiles cannot load four SIMDs evenly without a k split, and the longest
// wave has two tiles either way.  conv3 is 2 x 2 tiles, one per wave.
#pragma once
#include "cnn_layers.hpp"
#include "igemm_b3.hpp"

namespace {

constexpr size_t PL2_U16 = (size_t)3 * 64 * 512, PL3_U16 = (size_t)3 * 64 * 576;   // W2's / W3's three planes
// One parameter set's planes: W2 then W3, each [3 planes][K / 32][64 cout][32 k]: the B tile of k-tile kt (64 columns x 32 k of one plane) is
// 4 KB contiguous, so a wave of staging threads (16 columns x four 16-byte chunks) fetches 1 KB in one piece.  Measured against [cout][K] rows
// (+0.8 % on the step) and [K / 8][cout][8] (-1.8 %); k_reduce_adam's 32 consecutive cout of one k land 64 bytes apart.
constexpr size_t CPL_W2 = 0, CPL_W3 = PL2_U16, CPL_U16 = PL2_U16 + PL3_U16;
__device__ __forceinline__ size_t cpl_index(int k, int n) { return ((size_t)(k >> 5) * 64 + n) * 32 + (k & 31); }

// element e = k * 64 + n of W2 (layer 0) or W3 (layer 1) -> its three bf16 terms
__device__ __forceinline__ void conv_plane_store(uint16_t* __restrict__ pl, int layer, int e, float x)
{
    uint16_t v[3];
    split3_rn(x, v);                                            // (igemm_b3.hpp: round-to-nearest terms, exact sum)
    const size_t n = (size_t)(layer ? 576 : 512) * 64, o = cpl_index(e >> 6, e & 63);
    uint16_t* d = pl + (layer ? CPL_W3 : CPL_W2);
    d[o] = v[0]; d[n + o] = v[1]; d[2 * n + o] = v[2];
}

// the planes of one parameter set from its f32 weights (every writer of conv parameters other than k_reduce_adam leaves them stale:
// DqnCnn::cpl_fresh; the forward re-splits before it reads them)
__global__ __launch_bounds__(256) void k_conv_planes(const float* __restrict__ w2, const float* __restrict__ w3, uint16_t* __restrict__ pl)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 512 * 64) conv_plane_store(pl, 0, i, w2[i]);
    else if (i < 512 * 64 + 576 * 64) conv_plane_store(pl, 1, i - 512 * 64, w3[i - 512 * 64]);
}
// conv2 / conv3 forward, one launch per layer: the A rows are the f32 activations, split on their way into LDS; the weights are read
// from the bf16 planes (cpl_index)
#ifndef BDR_FWDC2_B3_SHAPE
#define BDR_FWDC2_B3_SHAPE 2, 2
#endif
#ifndef BDR_FWDC3_B3_SHAPE
#define BDR_FWDC3_B3_SHAPE 2, 2
#endif
struct FwdB3Args : FwdArgs { const uint16_t* wpl[MAXZ]; };
template <class G, int WM_, int WN_, int TM_ = 1, int TN_ = 1>
struct FwdB3 : FwdP<G, AFwd<G>, WM_, WN_, false, 0, TM_, TN_> {
    using Args = FwdB3Args;
    __device__ static const uint4* b_chunk(const Args& a, int z, int, int pl, int kt, int n, int kq)
    {
        return reinterpret_cast<const uint4*>(a.wpl[z] + (size_t)pl * G::COUT * G::K + cpl_index(kt * 32 + kq * 8, n));
    }
};
using FwdC2B3 = FwdB3<GeomC2, BDR_FWDC2_B3_SHAPE>;
using FwdC3B3 = FwdB3<GeomC3, BDR_FWDC3_B3_SHAPE>;

// ---- the fused launch ---------------------------------------------------------------------------------------------------------
struct FwdC23Args {
    const float* a1[MAXZ];        // [B][20][20][32]
    const uint16_t* cpl[MAXZ];    // the instance's planes (CPL_W2 / CPL_W3)
    const float* b2[MAXZ];
    const float* b3[MAXZ];
    float* a2[MAXZ];              // [B][9][9][64]
    float* a3[MAXZ];              // [B][7][7][64]
};

constexpr int C23_A1_BLK = 108;                        // pixels of one parity block of a1: 100 + the reach of the hole columns (95 + 11)
constexpr int C23_PL_A1 = 4 * C23_A1_BLK * 32;         // u16 per a1 plane
constexpr int C23_A2_PIX = 84;                         // 81 + the reach of the hole columns (63 + 20)
constexpr int C23_PL_A2 = C23_A2_PIX * 64;             // u16 per a2 plane
constexpr int C23_PL_W = 64 * B3_ROW, C23_W_STAGE = 3 * C23_PL_W;   // one k-tile of weights: 64 channels x 32 k per plane
constexpr int C23_NKT2 = GeomC2::K / BK, C23_NKT3 = GeomC3::K / BK, C23_NKT = C23_NKT2 + C23_NKT3;
constexpr int C23_LDS_U16 = 3 * C23_PL_A1 + 3 * C23_PL_A2 + 2 * C23_W_STAGE;
static_assert(C23_LDS_U16 * 2 <= 160 * 1024, "one workgroup per CU");
static_assert(C23_NKT2 % 2 == 0 && C23_NKT3 % 2 == 0, "the k loops are unrolled by two (stage and register set of a tile = its parity)");
__device__ __forceinline__ int c23_a1_off(int P, int c) { return P * 32 + ((c ^ ((P >> 2) & 3)) << 3); }
__device__ __forceinline__ int c23_a2_off(int P, int c) { return P * 64 + ((c ^ ((P >> 1) & 7)) << 3); }

// grid (B, 1, nz), 256 threads
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_fwd_c23_b3(FwdC23Args a)
{
    __shared__ __attribute__((aligned(16))) uint16_t smem[C23_LDS_U16];
    uint16_t* const sA1 = smem;
    uint16_t* const sA2 = sA1 + 3 * C23_PL_A1;
    uint16_t* const sW = sA2 + 3 * C23_PL_A2;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int img = blockIdx.x, z = blockIdx.z;
    using Set0 = std::integral_constant<int, 0>;
    using Set1 = std::integral_constant<int, 1>;
    using One = std::integral_constant<int, 1>;
    using Two = std::integral_constant<int, 2>;

    // ---- the weight stream: tile g of 34 (W2's 16, then W3's 18) lives in LDS stage g & 1 and, before that, in register set g & 1
    const uint16_t* const w2 = a.cpl[z] + CPL_W2 + tid * 8;
    const uint16_t* const w3 = a.cpl[z] + CPL_W3 + tid * 8;
    u32x4_t rb[2][3];
    auto wload = [&](auto set, int g) {
        constexpr int S = decltype(set)::value;
        g = min(g, C23_NKT - 1);
        const bool l2 = g < C23_NKT2;
        const uint16_t* p = l2 ? w2 + (size_t)g * C23_PL_W : w3 + (size_t)(g - C23_NKT2) * C23_PL_W;
        const size_t ps = l2 ? (size_t)64 * GeomC2::K : (size_t)64 * GeomC3::K;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) rb[S][pl] = *reinterpret_cast<const u32x4_t*>(p + pl * ps);
    };
    const int w_off = b3_off(tid >> 2, tid & 3);
    auto wcommit = [&](auto set, int stage) {
        constexpr int S = decltype(set)::value;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4_t*>(&sW[stage * C23_W_STAGE + pl * C23_PL_W + w_off]) = rb[S][pl];
    };

    // ---- prologue: the image and the first weight tiles in flight together
    constexpr int A1_V4 = 400 * 32 / 4, A1_PASSES = (A1_V4 + 255) / 256;
    f32x4 st[A1_PASSES];
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.a1[z] + (size_t)img * (400 * 32));
#pragma unroll
        for (int p = 0; p < A1_PASSES; ++p) st[p] = src[min(tid + 256 * p, A1_V4 - 1)];
    }
    wload(Set0{}, 0);
    wload(Set1{}, 1);
    // bias of this lane's channel runs [32 t + 8 q + 4 h, + 4)
    f32x4 bq2[2][4], bq3[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bq2[0][q] = *reinterpret_cast<const f32x4*>(a.b2[z] + 8 * q + 4 * h);
        bq2[1][q] = *reinterpret_cast<const f32x4*>(a.b2[z] + 32 + 8 * q + 4 * h);
        bq3[q] = *reinterpret_cast<const f32x4*>(a.b3[z] + 32 * (wave & 1) + 8 * q + 4 * h);
    }
#pragma unroll
    for (int p = 0; p < A1_PASSES; ++p) {
        const int i = tid + 256 * p;
        if (A1_V4 % 256 != 0 && i >= A1_V4) continue;
        const int pix = i >> 3, q4 = i & 7, ih = pix / 20, iw = pix - 20 * ih;
        const int P = ((ih & 1) * 2 + (iw & 1)) * C23_A1_BLK + (ih >> 1) * 10 + (iw >> 1);
        u32x2_t sp[3];
        split3_f32x4(st[p], sp);
        const int o = c23_a1_off(P, q4 >> 1) + (q4 & 1) * 4;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x2_t*>(&sA1[pl * C23_PL_A1 + o]) = sp[pl];
    }
    wcommit(Set0{}, 0);
    wload(Set0{}, 2);
    __syncthreads();

    f32x16 acc[2];
    bf16x8_t fx[2][3], fw[2][2][3];   // [fragment buffer]: the activation planes, the weight planes of up to two channel tiles
    // the fragments of k-step s of a tile: activations at sX[plane * plx + xoff], weights of channel tiles ct0 .. from `stage`
    auto load_frag = [&](auto buf, auto tn_, const uint16_t* sX, int plx, int xoff, int stage, int s, int ct0) {
        constexpr int F = decltype(buf)::value, TN = decltype(tn_)::value;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            fx[F][pl] = *reinterpret_cast<const bf16x8_t*>(&sX[pl * plx + xoff]);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                fw[F][tn][pl] = *reinterpret_cast<const bf16x8_t*>(&sW[stage * C23_W_STAGE + pl * C23_PL_W + b3_off((ct0 + tn) * 32 + j, s * 2 + h)]);
        }
    };
    // partial products, smallest first: (activation plane, weight plane) = ORD9[3..8] of k_igemm_b3
    auto mfma6 = [&](auto buf, auto tn_) {
        constexpr int F = decltype(buf)::value, TN = decltype(tn_)::value;
        constexpr int ORD[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                acc[tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[F][tn][ORD[t][1]], fx[F][ORD[t][0]], acc[tn], 0, 0, 0);
    };
    // One k-tile (two k-steps) of a layer.  par = parity of the tile in the stream of 34 (T0 and the loops are even, so also of kt):
    // its LDS stage; the other register set holds tile g + 1, which is committed to the other stage during the first k-step and
    // refilled with tile g + 3.  One barrier per tile, between the k-steps: by then every wave has committed tile g + 1 and has read
    // all of tile g (the fragments of a k-step are fetched one k-step ahead), so the second k-step can fetch tile g + 1's first
    // fragments and the next tile's commit may overwrite this stage.  xoff(kt, s): the lane's activation fragment.
    auto tile = [&](auto par, auto tn_, const uint16_t* sX, int plx, auto&& xoff, int T0, int kt, int nkt, bool active, int ct0) {
        constexpr int PAR = decltype(par)::value;
        using SetN = std::integral_constant<int, PAR ^ 1>;
        const int g = T0 + kt;
        if (active) load_frag(Set1{}, tn_, sX, plx, xoff(kt, 1), PAR, 1, ct0);
        if (g + 1 < C23_NKT) wcommit(SetN{}, PAR ^ 1);
        wload(SetN{}, g + 3);
        if (active) mfma6(Set0{}, tn_);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        if (active && kt + 1 < nkt) load_frag(Set0{}, tn_, sX, plx, xoff(kt + 1, 0), PAR ^ 1, 0, ct0);
        if (active) mfma6(Set1{}, tn_);
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- conv2: waves 0-2 = position tile `wave`, both channel tiles; column v = 10 oh + ow
    {
        const bool active = wave < 3;
        const int v = min(wave, 2) * 32 + j;
        auto xoff = [&](int kt, int s) {
            const int kh = kt >> 2, kw = kt & 3;
            return c23_a1_off(((kh & 1) * 2 + (kw & 1)) * C23_A1_BLK + v + 10 * (kh >> 1) + (kw >> 1), 2 * s + h);
        };
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tn][r] = 0.f;
        if (active) load_frag(Set0{}, Two{}, sA1, C23_PL_A1, xoff(0, 0), 0, 0, 0);
        for (int kt = 0; kt < C23_NKT2; kt += 2) {
            tile(Set0{}, Two{}, sA1, C23_PL_A1, xoff, 0, kt, C23_NKT2, active, 0);
            tile(Set1{}, Two{}, sA1, C23_PL_A1, xoff, 0, kt + 1, C23_NKT2, active, 0);
        }
        const int oh = v / 10, ow = v - 10 * oh;
        if (active && oh < 9 && ow < 9) {
            const int m = oh * 9 + ow;
            float* out = a.a2[z] + ((size_t)img * 81 + m) * 64 + 4 * h;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float t = acc[tn][4 * q + e] + bq2[tn][q][e]; y[e] = t > 0.f ? t : 0.f; }   // FwdP::store
                    *reinterpret_cast<f32x4*>(out + 32 * tn + 8 * q) = y;
                    u32x2_t sp[3];
                    split3_f32x4(y, sp);
                    const int o = c23_a2_off(m, 4 * tn + q) + 4 * h;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x2_t*>(&sA2[pl * C23_PL_A2 + o]) = sp[pl];
                }
        }
    }
    __syncthreads();   // a2 is complete in LDS (W3's first tile was committed in front of conv2's last barrier)

    // ---- conv3: wave = (position tile, channel tile); column v = 9 oh + ow
    {
        const int v = (wave >> 1) * 32 + j, ct = wave & 1;
        auto xoff = [&](int kt, int s) {
            const int tap = kt >> 1, kh = tap / 3, kw = tap - 3 * kh;
            return c23_a2_off(v + 9 * kh + kw, (kt & 1) * 4 + 2 * s + h);
        };
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = 0.f;
        load_frag(Set0{}, One{}, sA2, C23_PL_A2, xoff(0, 0), 0, 0, ct);
        for (int kt = 0; kt < C23_NKT3; kt += 2) {
            tile(Set0{}, One{}, sA2, C23_PL_A2, xoff, C23_NKT2, kt, C23_NKT3, true, ct);
            tile(Set1{}, One{}, sA2, C23_PL_A2, xoff, C23_NKT2, kt + 1, C23_NKT3, true, ct);
        }
        const int oh = v / 9, ow = v - 9 * oh;
        if (oh < 7 && ow < 7) {
            float* out = a.a3[z] + ((size_t)img * 49 + oh * 7 + ow) * 64 + 32 * ct + 4 * h;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 y;
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float t = acc[0][4 * q + e] + bq3[q][e]; y[e] = t > 0.f ? t : 0.f; }
                *reinterpret_cast<f32x4*>(out + 8 * q) = y;
            }
        }
    }
}

inline hipError_t launch_fwd_c23_b3(hipStream_t st, int B, int nz, const FwdC23Args& args)
{
    hipLaunchKernelGGL(k_fwd_c23_b3, dim3(B, 1, nz), dim3(256), 0, st, args);
    return hipGetLastError();
}

}  // namespace
