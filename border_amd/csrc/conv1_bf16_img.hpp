// conv1 forward, third form: the input images staged through LDS as bf16, the output stored as 16-byte vectors.
//
// Same arithmetic as conv1_bf16.hpp (u8 pixels exact in bf16, every f32 weight split exactly into three bf16 terms, products exact,
// f32 accumulation in the MFMA; per output the same k-steps in the same order: 16 k per step, planes lo, mid, hi): bit-identical
// results (tools/probes/conv1_rw_probe.hip compares the words).  What differs is what the kernel asks of the memory pipes:
//  * a workgroup copies its image(s) into LDS with coalesced 16-byte loads (1 764 per n_stack = 4 image instead of 200 overlapping
//    eight-byte gathers per 32-pixel unit, every pixel fetched four times) and converts every pixel to bf16 ONCE on the way (the
//    first form converted it once per fragment: ~4 VALU operations per MFMA in the item loop).  A fragment - 8 pixels of a patch row -
//    is 16 bytes at an 8-byte aligned LDS address (ds_read2_b64); pixel m of an image sits at dword 2 m + 128 oh of its plane, so the
//    32 lanes of a half wave always fall into different banks;
//  * the MFMA operand roles are swapped - rows = the 32 output channels, columns = 32 pixels - so a lane ends up with four runs of 4
//    CONSECUTIVE channels of one pixel: the NHWC epilogue is 4 global_store_dwordx4 per unit instead of 16 dword stores (the MFMA
//    computes D^T = B^T A^T element by element: same sums);
//  * IPW images per workgroup pass (1 or 2): with two images the units of a pass spread more evenly over the waves.
// NT threads = NT / 64 waves take the pass's 32-pixel units round robin; the weight fragments are read from LDS one k-step ahead, the
// pixel fragments two.  Measured and dropped (tools/probes/conv1_rw_probe.hip, conv1_bf16_rw.hpp): the weight planes in REGISTERS with one
// wave per SIMD and two or four accumulator chains per wave (11.3 us: an in-order wave pays ~12 cycles of matrix-pipe time for every LDS
// read it issues between its MFMAs, two waves per SIMD hide them), two units per wave with shared weight fragments (10.1), the
// un-swapped roles with sixteen full-row dword stores (9.4-10.0: no difference).  Where the launch's 9.6 us are at one instance of
// B = 256 (stamps of the probe): ~1.8 launch, 3.2 until the first MFMA (first-touch loads of image and weights, split, conversion,
// barrier), ~2.3 of MFMAs with the 13 units of an image spread 4 / 3 / 3 / 3 over the SIMDs, ~2.3 for the 13 MB of stores, which
// only start when the first units are done.  cnn/base.rs:26-28.
#pragma once
#include <algorithm>
#include <cstdlib>
#include "conv1_bf16.hpp"

namespace bdr {

constexpr int C1IMG_MAX_STACK = 6;   // bf16 image (14 112 B per frame) + three weight planes (12 KiB per frame) in 160 KB of LDS

#ifdef C1_TRACE   // tools/probes only: wall-clock stamps (100 MHz) of the first and the last wave of every workgroup
__device__ unsigned long long* g_c1_trace;
#define C1_TP(slot) do { if ((threadIdx.x & 63) == 0 && g_c1_trace && ((threadIdx.x >> 6) == 0 || (threadIdx.x >> 6) == (blockDim.x >> 6) - 1)) { unsigned long long* t__ = g_c1_trace + (blockIdx.x * 2 + ((threadIdx.x >> 6) ? 1 : 0)) * 8; t__[slot] = wall_clock64(); if ((slot) == 4) t__[5] = clock64(); if ((slot) == 6) t__[7] = clock64(); } } while (0)
#else
#define C1_TP(slot) do { } while (0)
#endif

template <int NS, int IPW, int NT>
static __global__ __launch_bounds__(NT, NT / 256) void k_conv1_bf16_img(Conv1Args a)
{
#include "conv1_bf16_img_body_inc.hpp"
}

// waves = 8 or 16 per workgroup
inline hipError_t launch_conv1_bf16_img(int ns, int ipw, int waves, dim3 grid, hipStream_t st, const Conv1Args& c)
{
    if (ns < 1 || ns > C1IMG_MAX_STACK || ipw < 1 || ipw > 2 || (waves != 8 && waves != 16) || (ns > 4 && ipw == 2)) return hipErrorInvalidValue;
    switch (ns * 4 + (ipw - 1) * 2 + (waves == 16)) {
#define BDR_C1IMG_CASE1(N) \
        case N * 4 + 0: hipLaunchKernelGGL((k_conv1_bf16_img<N, 1, 512>), grid, dim3(512), 0, st, c); break; \
        case N * 4 + 1: hipLaunchKernelGGL((k_conv1_bf16_img<N, 1, 1024>), grid, dim3(1024), 0, st, c); break;
#define BDR_C1IMG_CASE(N) BDR_C1IMG_CASE1(N) \
        case N * 4 + 2: hipLaunchKernelGGL((k_conv1_bf16_img<N, 2, 512>), grid, dim3(512), 0, st, c); break; \
        case N * 4 + 3: hipLaunchKernelGGL((k_conv1_bf16_img<N, 2, 1024>), grid, dim3(1024), 0, st, c); break;
        BDR_C1IMG_CASE(1) BDR_C1IMG_CASE(2) BDR_C1IMG_CASE(3) BDR_C1IMG_CASE(4) BDR_C1IMG_CASE1(5) BDR_C1IMG_CASE1(6)
#undef BDR_C1IMG_CASE
#undef BDR_C1IMG_CASE1
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// conv1 forward of nz network instances on B images each: the staged-image form where its LDS image fits (bf16 image(s) + three weight
// planes <= 160 KB: n_stack <= 6, two images per pass up to n_stack 4), the direct form of conv1_bf16.hpp otherwise.  Same bits either way.
// BDR_C1_FORM (diagnostic, read once): -1 = always the direct form, 8 / 16 = waves per workgroup of the staged form (default 8).
inline int conv1_form_env()
{
    static const int form = [] { const char* e = getenv("BDR_C1_FORM"); return e ? atoi(e) : 8; }();
    return form;
}
inline hipError_t conv1_forward(int ns, int B, hipStream_t st, const Conv1Args& c, int cus = 256)
{
    const int form = conv1_form_env();
    if (ns <= C1IMG_MAX_STACK && form >= 0 && c.M == B * 400) {
        const int per_inst = std::max(1, cus / c.nz);
        const int ipw = (ns <= 4 && B > per_inst) ? 2 : 1;
        const int g = std::max(1, std::min(per_inst, (B + ipw - 1) / ipw));
        return launch_conv1_bf16_img(ns, ipw, form == 16 ? 16 : 8, dim3(g * c.nz), st, c);
    }
    const int items = (c.M + 31) / 32;
    const int g = std::max(1, std::min(512 / c.nz, (items + 7) / 8));
    return launch_conv1_bf16(ns, dim3(g * c.nz), st, c);
}

}  // namespace bdr
