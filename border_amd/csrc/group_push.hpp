// ================================================================================================
// The grouped push of the groups on group_core.hpp (bdr_awac_group_push, bdr_candle_sac_group_push): ExperienceBufferBase::push
// (generic_replay_buffer/base.rs:279-313) of n transitions per member into the member's own ring, ONE launch and no copy command
// whatever P and n are.  The device half; the host half is group_push<G> in group_core.hpp.
// A slot of the group's pinned, device-mapped push ring holds [CGroupPushDesc[P] | member 0's n records | member 1's n records | ...].
//   F32 rows   a record is laid out exactly as bdr_replay_push lays it out for that ring (obs | next_obs | act | reward, flags at
//              the ring's own offsets) and is a multiple of 16 bytes like its destination `ring + row * stride`, so source and
//              destination of every field share their alignment and take gp_copy's 16-byte / 4-byte / byte lanes (gp_copy.hpp,
//              shared with k_group_push)
//   F64 rows   obs and next_obs are staged raw (8 bytes an element, each block padded to 16 bytes); act and the tail follow at
//              the ring's own offsets modulo 16.  The kernel stores (float)x per element: one round-to-nearest-even conversion, the
//              cast the acting kernel applies to the same rows (dense_act.hpp) and numpy's astype(float32).  No normaliser.
// One wave per (member, row), four waves per workgroup: wave w = member * n + row, grid = ceil(P n / 4) workgroups of 256 threads.
// Row j of member i goes to ring row (head_i + j) % capacity_i.  When n exceeds a ring's capacity, rows j and j + capacity name one
// ring row and a standalone push leaves the later one: only rows with j + capacity >= n are written, so no two waves share a row.
// Exactly the bytes a standalone push defines are written: the two rows, act_bytes, reward and two flags.
// Bounds: w < P n selects a descriptor p < P and a record j < n; the host has checked src_off + n * rec_bytes <= the slot's size and
// s_tail_off + 8 <= rec_bytes; the ring row is < capacity and tail_off + 6 <= stride (the ring's own layout).  Plain vector loads
// and stores, the agent-scope atomics of the ticket: nothing new.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gp_copy.hpp"
#include "group_done.hpp"

struct CGroupPushDesc {
    uint8_t* ring; uint64_t head, capacity, stride;                      // the ring at call time: row j goes to (head + j) % capacity
    uint32_t src_off, rec_bytes;                                         // the member's n records in the slot, rec_bytes apart
    uint32_t obs_bytes, act_bytes, next_off, act_off, tail_off;          // the ring's layout (obs_bytes = 4 * obs_dim)
    uint32_t s_next_off, s_act_off, s_tail_off;                          // the staged record's layout (obs at 0)
    uint32_t f64, pad;                                                   // 1: obs / next_obs staged as float64
};
static_assert(sizeof(CGroupPushDesc) == 80, "CGroupPushDesc is read in 16-byte pieces");

namespace {

// n_elem float64 -> f32 by one wave: one round-to-nearest-even conversion per element
__device__ __forceinline__ void gp_cast_f64(uint8_t* dst, const uint8_t* src, uint32_t n_elem, int lane)
{
    for (uint32_t i = lane; i < n_elem; i += 64) reinterpret_cast<float*>(dst)[i] = (float)reinterpret_cast<const double*>(src)[i];
}

__global__ __launch_bounds__(256) void k_cgroup_push(const uint8_t* __restrict__ slot, unsigned P, unsigned n, unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    const int lane = threadIdx.x & 63;
    const unsigned w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w < P * n) {
        const unsigned p = w / n, j = w - p * n;
        const CGroupPushDesc d = reinterpret_cast<const CGroupPushDesc*>(slot)[p];
        if ((uint64_t)j + d.capacity >= n) {   // (a later row of this call takes the ring row otherwise)
            const uint8_t* rec = slot + d.src_off + (size_t)j * d.rec_bytes;
            uint8_t* dst = d.ring + ((d.head + j) % d.capacity) * d.stride;
            if (d.f64) {
                gp_cast_f64(dst, rec, d.obs_bytes / 4, lane);
                gp_cast_f64(dst + d.next_off, rec + d.s_next_off, d.obs_bytes / 4, lane);
            } else {
                gp_copy(dst, rec, d.obs_bytes, lane);
                gp_copy(dst + d.next_off, rec + d.s_next_off, d.obs_bytes, lane);
            }
            gp_copy(dst + d.act_off, rec + d.s_act_off, d.act_bytes, lane);
            gp_copy(dst + d.tail_off, rec + d.s_tail_off, 6, lane);   // reward f32, is_terminated, is_truncated
        }
    }
    bg_group_done(ticket, seq_host, seq);   // every wave's loads of the slot have returned: their data went into the stores above
}

}  // namespace
