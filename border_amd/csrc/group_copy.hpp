// ================================================================================================
// Copying training state between members of a group on group_core.hpp (bdr_bc_group_copy_members, bdr_iql_group_copy_members,
// bdr_awac_group_copy_members, bdr_candle_sac_group_copy_members): any list of (source -> destination) pairs in ONE launch and no copy
// command, event or synchronise - the exploit step of population-based training, successive halving's "survivors overwrite the dropped".
// All members of a group have one shape, so the arenas a member lists (DenseAgent::state_arenas: every arena its model table serves -
// online and target networks, the last gradient, exp_avg, exp_avg_sq; the candle SAC's entropy block with log_alpha, its gradient, its
// moments and alpha) correspond one to one between two members.
// A segment is one (pair, arena): {src, dst, n4} with n4 = the arena's length in 16-byte vectors.  The host writes the call's segments
// into a slot of a pinned, device-mapped ring under the slot rule of slot_ring.hpp; k_group_copy reads the slot in place (grid y = the
// segment: uniform, so its three words are scalar loads), is its only reader, ends with the group's done ticket and publishes its launch
// number, which it takes from the group's counter as the push kernel does (group_done.hpp).
// Every arena is a multiple of 4 floats by construction (MlpLayout pads both dimensions of every layer to 64, head2 to pad64(A), the
// entropy block holds 8 floats) and 256-byte aligned (hipMalloc): the host states it with a BDR_REQUIRE and the kernel has no tail.
// Bounds: y = blockIdx.y < gridDim.y = the number of segments written to the slot <= GC_MAX_SEGS = 65535 = what grid y holds, and <=
// the slot's capacity (P - 1) x arenas: a valid list has at most P - 1 pairs.  Vector j < n4 of a segment only.  No member is read and
// written by one call (the host refuses a member that is a destination in one pair and a source in another, and a destination listed
// twice), so no segment's stores meet another segment's loads or stores and the kernel needs no ordering inside.  Plain vector loads
// and stores, the agent-scope atomics of the ticket: nothing new.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <vector>

#include "group_done.hpp"

struct GroupCopySeg { const float* src; float* dst; unsigned long long n4, pad; };
static_assert(sizeof(GroupCopySeg) == 32, "GroupCopySeg is laid out in pinned slots");

namespace {

constexpr unsigned GC_MAX_SEGS = 65535;   // grid dimension y
constexpr int GC_SLOTS = 8;               // slots of the pinned segment ring
constexpr int GC_INFLIGHT = 4;            // 16-byte loads a lane has in flight before its stores
constexpr unsigned GC_MAX_GX = 64;        // workgroups walking one segment, at most

// grid (workgroups per segment, segments): workgroup x of segment y moves vectors x * 256 + lane, + gridDim.x * 256, ... of the segment,
// GC_INFLIGHT loads before their stores
__global__ __launch_bounds__(256) void k_group_copy(const BDR_CONST_AS GroupCopySeg* segs, unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    const BDR_CONST_AS GroupCopySeg& s = segs[blockIdx.y];
    const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(s.src);
    f32x4* __restrict__ dst = reinterpret_cast<f32x4*>(s.dst);
    const size_t n4 = s.n4, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride * GC_INFLIGHT) {
        f32x4 v[GC_INFLIGHT];
#pragma unroll
        for (int u = 0; u < GC_INFLIGHT; ++u)
            if (i + u * stride < n4) v[u] = src[i + u * stride];
#pragma unroll
        for (int u = 0; u < GC_INFLIGHT; ++u)
            if (i + u * stride < n4) dst[i + u * stride] = v[u];
    }
    bg_group_done(ticket, seq_host, seq);   // every thread's loads of the slot have returned: their addresses went into the stores above
}

// ---- host: every refusal, then the slot, the launch, and the host half of every pair ---------------------------------------------------
// (G: a GroupCore<K> whose members are DenseAgents; flags: BDR_COPY_HYPER)
template <class G>
int32_t group_copy_members(G* g, const uint32_t* src, const uint32_t* dst, uint32_t n, uint32_t flags)
{
    BDR_REQUIRE(g && src && dst, "null argument");
    BDR_REQUIRE((flags & ~(uint32_t)BDR_COPY_HYPER) == 0, "unknown copy flags 0x%x", flags);
    BDR_REQUIRE(n >= 1, "a copy takes at least one (source, destination) pair (n = 0)");
    const uint32_t P = (uint32_t)g->members.size();
    std::vector<DenseAgent::StateArena> as, ad;
    g->members[0]->state_arenas(as);
    const size_t na = as.size();
    BDR_REQUIRE(na >= 1 && (uint64_t)n * na <= GC_MAX_SEGS, "%u pairs of %u arenas each are %llu segments, one launch takes %u (grid dimension y): split the call", n,
                (unsigned)na, (unsigned long long)n * na, GC_MAX_SEGS);
    std::vector<uint8_t> role(P, 0);   // 1: a source, 2: a destination
    for (uint32_t i = 0; i < n; ++i) {
        BDR_REQUIRE(src[i] < P && dst[i] < P, "pair %u (%u -> %u): a group of %u members has no member %u", i, src[i], dst[i], P, src[i] < P ? dst[i] : src[i]);
        BDR_REQUIRE(src[i] != dst[i], "pair %u (%u -> %u): source and destination are one member", i, src[i], dst[i]);
        BDR_REQUIRE(role[dst[i]] != 2, "pair %u (%u -> %u): member %u is the destination of an earlier pair", i, src[i], dst[i], dst[i]);
        BDR_REQUIRE(role[dst[i]] != 1, "pair %u (%u -> %u): member %u is the source of another pair: no member is read and written by one call", i, src[i], dst[i], dst[i]);
        BDR_REQUIRE(role[src[i]] != 2, "pair %u (%u -> %u): member %u is the destination of another pair: no member is read and written by one call", i, src[i], dst[i],
                    src[i]);
        role[src[i]] = 1; role[dst[i]] = 2;
    }
    BDR_HIP(hipSetDevice(g->device));
    const size_t slot_segs = std::min<size_t>(GC_MAX_SEGS, (size_t)(P - 1) * na);   // (n <= P - 1: the destinations differ and none is a source)
    if (!g->copy.host) BDR_HIP(pinned_array(g->copy, (size_t)GC_SLOTS * slot_segs));   // the first copy
    const auto slot = g->copy_ring.next();
    if (slot.wait) {   // the slot's last reader has published (bounded: wait_seq_word)
        bool arrived = false;
        BDR_TRY(wait_seq_word(g->seq.host.get(), (unsigned)slot.wait, g->stream, std::chrono::steady_clock::now(), &arrived));
    }
    GroupCopySeg* segs = g->copy.host.get() + (size_t)slot.slot * slot_segs;
    size_t ns = 0, max_n4 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        g->members[src[i]]->state_arenas(as);
        g->members[dst[i]]->state_arenas(ad);
        BDR_REQUIRE(as.size() == na && ad.size() == na, "pair %u (%u -> %u): the members list different arenas", i, src[i], dst[i]);
        for (size_t k = 0; k < na; ++k) {
            BDR_REQUIRE(as[k].n == ad[k].n && as[k].n % 4 == 0 && as[k].p && ad[k].p && (uintptr_t)as[k].p % 16 == 0 && (uintptr_t)ad[k].p % 16 == 0,
                        "pair %u (%u -> %u): arena %u holds %llu and %llu floats: one length, a multiple of 4 floats, 16-byte aligned", i, src[i], dst[i], (unsigned)k,
                        (unsigned long long)as[k].n, (unsigned long long)ad[k].n);
            segs[ns++] = GroupCopySeg{as[k].p, ad[k].p, (unsigned long long)(as[k].n / 4), 0};
            max_n4 = std::max(max_n4, as[k].n / 4);
        }
    }
    std::atomic_thread_fence(std::memory_order_release);
    // (should the launch fail, k is the number of whatever the group launches next - later than every reader of the slot)
    const uint64_t k = g->launches + 1;
    g->launches = k; g->copy_ring.record(k);
    const unsigned gx = (unsigned)std::min<size_t>(GC_MAX_GX, std::max<size_t>(1, (max_n4 + 256 * GC_INFLIGHT - 1) / (256 * GC_INFLIGHT)));
    hipLaunchKernelGGL(k_group_copy, dim3(gx, (unsigned)ns), dim3(256), 0, g->stream, (const BDR_CONST_AS GroupCopySeg*)(g->copy.dev + (size_t)slot.slot * slot_segs),
                       g->ticket.get(), g->seq.dev, (unsigned)k);
    BDR_HIP(hipGetLastError());
    g->kernel_launches += 1;
    // the host half: step counters (and with BDR_COPY_HYPER the settable hyperparameters) follow; seed, noise counter, mode, act
    // path, buffer and index stream, n_opts and evaluator bookkeeping stay the destination's
    for (uint32_t i = 0; i < n; ++i) g->members[dst[i]]->state_adopt(*g->members[src[i]], (flags & BDR_COPY_HYPER) != 0);
    return BDR_OK;
}

}  // namespace
