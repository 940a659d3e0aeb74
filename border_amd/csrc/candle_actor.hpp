// Device helpers shared by the candle-family agents (IQL, AWAC): the counter-based N(0,1) noise stream of Policy::sample and the
// fixed-order batch sums.  Every batch-wide sum is formed in one order (rows in blocks of 32, a 32-lane butterfly per block, the
// block partials added in block order), so an update gives the same bits run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>

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
__device__ __forceinline__ float acc(float base, float s, float scale)   // base + s * scale, rounded step by step
{
#pragma clang fp contract(off)
    const float t = s * scale;
    return base + t;
}

}  // namespace candle
}  // namespace bdr
