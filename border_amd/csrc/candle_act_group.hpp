// ================================================================================================
// Group acting of Gaussian actors: Policy::sample (util/actor.rs:226-241) of the selected members of a group in ONE launch.
// k_candle_act_group<TEAMS> runs dense_act_body (dense_act.hpp) in its candle-only form, DA_EPI_CANDLE, with the selected member as
// grid dimension y, as k_bc_act_group (bc_group.hpp) runs the BC-only form.  Nothing here names an agent kind: the entry works on
// DenseActArgs[P] (the network and the STATIC half of the element code's operands - head2, the log-std clamps, the action limit, seed,
// mlp2 - in the group's device array, rewritten only when a member's actor arena has moved), CandleActCall[P] (the words of THIS call
// - the member's staged rows, its result block, and the per-call half of the operands: train and counter - in pinned, device-mapped
// memory) and `sel`.  Both arrays are read in place through the constant address space: member = sel[blockIdx.y] is uniform, so the
// member's fields stay scalar loads.  The body builds the SampleElem of candle_sample_elem in registers from the two halves, z null.
//   Bits.  Same body, same tile order, same element code as the member's own k_dense_act; element t = (m0 + rr) * A + j of the member's
//   own call draws at counter + t, so with `counter` = the member's noise counter the actions are those of its own
//   bdr_agent_sample_raw in the mode it is in, at the counter it is at.  Members of one call may be in different modes.
//   Mlp2 actors.  The operand cur[rr * ldz + A + j] is the shared expression of the body; no group hands this entry an Mlp2 actor yet
//   (the host writes mlp2 = 0), so that form is not reached under a group and nothing is claimed for it.
//   The end.  An acting call is synchronous: every thread's result stores are fenced at system scope, then the launch counts its
//   workgroups on the group's ticket and publishes its launch number (bg_group_done); the host waits for that number before it reads
//   the results.  Stores are plain vector stores.
//   Bounds of every new index.  y = blockIdx.y < gridDim.y = the number of selected members = the length of `sel` that the host has
//   written; member = sel[y] < P = the length of `args` and `calls` (checked by the host before anything is enqueued).  x =
//   blockIdx.x < gridDim.x = ceil(n / 32) row blocks of ONE member's call, n = calls[member].n, the same for every selected member.
//   Inside a member every index is the body's own, with the standalone kernel's bounds: rows are read for m0 + r < n and c < O from the
//   member's staged block of n * O elements, out is written at t = (m0 + r) * A + j < n * A inside the member's block of n * A floats,
//   head2 is read at j < A of the member's actor arena, the draw index counter + t is a 64-bit sum.
#pragma once
#include "group_done.hpp"

namespace {

// BcActCall's words (group_act.hpp reads the common ones by name), then the per-call half of SampleElem
struct CandleActCall {
    const uint8_t* rows; unsigned long long row_stride; const float* mean; const float* std; float* out; long long* idx; int n, f64;
    int train; unsigned long long counter;
};

template <int TEAMS>
__global__ __launch_bounds__(256 * TEAMS) void k_candle_act_group(const BDR_CONST_AS DenseActArgs* args, const BDR_CONST_AS CandleActCall* calls,
                                                                  const BDR_CONST_AS unsigned* sel, unsigned* ticket, unsigned* seq_host, unsigned seq)
{
    extern __shared__ __attribute__((aligned(16))) float da_lds[];
    const unsigned member = sel[blockIdx.y];
    dense_act_body<TEAMS, DA_EPI_CANDLE>(args[member], calls[member], da_lds);
    __threadfence_system();   // this thread's result rows are in host memory before its workgroup counts
    bg_group_done(ticket, seq_host, seq);
}

}  // namespace
