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
//   Mlp2 actors (candle_sac_group.hpp hands this entry members whose actor is one: the host writes the member's own form, mlp2 = 1 and
//   a null head2, which the element code does not read in that form).  The last layer is [mean | s] of logical width 2 A, padded to
//   Np = pad64(2 A) >= 2 A, and the epilogue reads s at cur[rr * ldz + A + j] with rr < rows_here <= 32, j < A, so A + j < 2 A <= Np <
//   ldz = Np + 4: inside row rr of the [32][Np + 4] buffer.  LDS is sized by W = the widest padded layer of the member (act_width:
//   the maximum of every layer's Kp and Np, the last layer's pad64(2 A) included), two [32][W + 4] buffers, so ldz <= W + 4 and the
//   rows fit; the host refuses W > DA_MAX_W before anything is enqueued.  IQL and AWAC members are Mlp3 actors and still get mlp2 = 0.
//   The end.  An acting call is synchronous: every thread's result stores are fenced at system scope, then the launch counts its
//   workgroups on the group's ticket and publishes its launch number (bg_group_done); the host waits for that number before it reads
//   the results.  Stores are plain vector stores.
//   Bounds of every new index.  y = blockIdx.y < gridDim.y = the number of selected members = the length of `sel` that the host has
//   written; member = sel[y] < P = the length of `args` and `calls` (checked by the host before anything is enqueued).  x =
//   blockIdx.x < gridDim.x = ceil(n / 32) row blocks of ONE member's call, n = calls[member].n, the same for every selected member.
//   Inside a member every index is the body's own, with the standalone kernel's bounds: rows are read for m0 + r < n and c < O from the
//   member's staged block of n * O elements, out is written at t = (m0 + r) * A + j < n * A inside the member's block of n * A floats,
//   head2 is read at j < A of the member's actor arena, the draw index counter + t is a 64-bit sum.
//   The host half.  CandleActKind<M> below is what group_act.hpp's call needs of a kind, written once over the CandleAgent member M
//   (candle_actor.hpp: Iql, Awac, CandleSac).
#pragma once
#include "group_done.hpp"
#include "group_act.hpp"

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

// ---- group acting of CandleAgent members: group_act.hpp's call with what is a Gaussian actor's ----------------------------------------
// Static, keyed on the actor arena: the actor net pn on pi_p, DA_CANDLE, and the static half of CandleAgent::sample_elem from the
// member's config and actor form (Mlp3 for IQL and AWAC members: mlp2 = 0; a candle SAC member may be Mlp2).  Per call: the member's mode, read now (bdr_agent_set_train), and in train
// mode its noise counter, which advances by the n * A draws the call takes - sample_elem's rule, so group calls, group rounds that draw
// (awac_group.hpp), the member's own sample / sample_raw on either act path and bdr_agent_noise continue one stream in any
// interleaving.  The call does not go through ensure_batch and does not touch a member's samp: results go to the group's pinned area.
template <class M>
struct CandleActKind : GroupActEntry<CandleActCall, k_candle_act_group<1>, k_candle_act_group<2>> {
    const float* arena(const M* m) const { return m->pi_p; }
    void write_static(const M* m, DenseActArgs& a) const
    {
        const MlpLayout& pn = m->pn;
        a.nl = (int)pn.L.size();
        for (int l = 0; l < a.nl; ++l) a.L[l] = DenseActLayer{m->pi_p + pn.L[l].w, m->pi_p + pn.L[l].b, pn.L[l].Kp, pn.L[l].Np, pn.L[l].relu};
        a.mode = DA_CANDLE;
        SampleElem& e = a.e;   // train, counter and z are the call's
        e.mlp2 = m->mlp2() ? 1 : 0; e.head2 = e.mlp2 ? nullptr : m->pi_p + m->h2_off;   // the member's actor form; Mlp2 has no head2
        e.lo = (float)m->cfg.min_log_std; e.hi = (float)m->cfg.max_log_std; e.tanh_limit = m->cfg.action_limit == BDR_ACTION_LIMIT_TANH ? 1 : 0;
        e.amin = (float)m->cfg.action_min; e.amax = (float)m->cfg.action_max; e.scale = (float)m->cfg.action_scale;
        e.seed = m->cfg.seed;
    }
    void noise(const M* m, int* train, uint64_t* counter) const { *train = m->train ? 1 : 0; *counter = m->noise_counter; }
    void call_words(M* m, CandleActCall& c, int train, uint64_t start, uint64_t counter) const
    {
        c.train = train; c.counter = train ? start : 0;
        m->noise_counter = counter;
    }
};

}  // namespace
