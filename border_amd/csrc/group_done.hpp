// The end-of-round ticket of the launch groupings of dense agents (bc_group.hpp: BC; iql_group.hpp: IQL; awac_group.hpp: AWAC), gl_group_done's rule
// (group_layers.hpp): the last launch of a round that reads the step slot calls it as its last statement.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// every workgroup of the launch counts, behind a barrier every thread reaches; the last one re-arms the ticket and publishes the
// launch number to the pinned word (slot_ring.hpp)
__device__ __forceinline__ void bg_group_done(unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x * gridDim.y * gridDim.z - 1) {
        atomicExch(ticket, 0u);   // (the next launch is behind this one in the stream)
        __hip_atomic_store(seq_host, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace
