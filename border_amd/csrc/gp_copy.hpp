// The copy lanes of the grouped pushes (k_group_push, agent_group.hpp; k_cgroup_push, group_push.hpp): one wave moves one field of
// one record from a pinned staging slot into a ring row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// n bytes by one wave: 16-byte lanes, then 4-byte lanes over what is left, then single bytes (rows of 12 and 24 bytes take the 4-byte lanes)
__device__ __forceinline__ void gp_copy(uint8_t* dst, const uint8_t* src, uint32_t n, int lane)
{
    uint32_t done = 0;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const uint32_t nv = n / 16;
        for (uint32_t i = lane; i < nv; i += 64) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        done = nv * 16;
    }
    if ((((uintptr_t)src | (uintptr_t)dst) & 3) == 0) {
        const uint32_t nw = (n - done) / 4;
        for (uint32_t i = lane; i < nw; i += 64) reinterpret_cast<uint32_t*>(dst + done)[i] = reinterpret_cast<const uint32_t*>(src + done)[i];
        done += nw * 4;
    }
    for (uint32_t i = done + lane; i < n; i += 64) dst[i] = src[i];
}
