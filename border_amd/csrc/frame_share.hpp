// The sharing rule of the single-frame store (bdr_replay_config::frame_stack), apart from where the bytes live: which frames of an
// incoming transition reuse a stored frame, which get a new sequence number, and when the store is exhausted.  Host only, no HIP:
// the host push (replay.hip push_frames) answers the equality questions with memcmp on the caller's rows, the device push
// (bdr_replay_push_device_frames) with the flags k_frame_eq computed in HBM - one procedure, so the two cannot drift apart.
//
// Frames are newest first (border-atari-env/src/env.rs:197-209 stack_frame), k = frame_stack.  The 4k - 3 questions of a transition:
//   P[j]  j < k      obs frame j      == frame j of the previous push's next_obs     (all k: the episode continues, obs costs nothing)
//   A[j]  j < k - 1  obs frame j      == obs frame j + 1                             (reset stack, env.rs:263-296: stored once)
//   S[j]  j < k - 1  next_obs frame j + 1 == obs frame j                             (all k - 1: next_obs costs its newest frame only)
//   N[j]  j < k - 1  next_obs frame j == next_obs frame j + 1
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace bdr {

inline int frame_q_count(int k) { return 4 * k - 3; }
inline int frame_q_P(int, int j) { return j; }
inline int frame_q_A(int k, int j) { return k + j; }
inline int frame_q_S(int k, int j) { return 2 * k - 1 + j; }
inline int frame_q_N(int k, int j) { return 3 * k - 2 + j; }

struct FrameShare {
    int k = 0;                              // frames per observation
    uint64_t capacity = 0, frame_cap = 0;   // transitions in the ring, frames in the store (slot = sequence number % frame_cap)
    uint64_t frame_seq = 0;                 // frames allocated so far
    std::vector<uint64_t> first_ref;        // per transition slot: smallest frame sequence number it references
    std::vector<uint64_t> last_next_seq;    // sequence numbers of the last pushed next_obs' k frames
    bool have_last = false;
    std::vector<uint64_t> oseq, nseq;       // the transition frame_share_step placed last: sequence numbers of its obs / next_obs frames

    void init(int k_, uint64_t capacity_, uint64_t frame_cap_)
    {
        k = k_; capacity = capacity_; frame_cap = frame_cap_; frame_seq = 0; have_last = false;
        first_ref.assign(capacity, 0); last_next_seq.assign(k, 0); oseq.assign(k, 0); nseq.assign(k, 0);
    }
};

// Places one transition: ring slot `pos`, `pushed` transitions went in before it (the buffer's size plus those of this call;
// anything >= capacity means the ring is full).  eq(q) answers question q (asked lazily: what is not asked does not matter);
// on_alloc(src, j, seq) is told that frame j of obs (src 0) / next_obs (src 1) is new and gets sequence number seq - in increasing
// seq, without gaps.  Frames are allocated in push order in a ring of frame_cap slots; a slot may only be reused once no live
// transition references it.
// false: the store is exhausted - f.first_ref / last_next_seq / have_last are untouched, f.frame_seq keeps what this transition
// had been given before it failed (those slots hold no live frame).
template <class Eq, class OnAlloc>
inline bool frame_share_step(FrameShare& f, uint64_t pos, uint64_t pushed, Eq&& eq, OnAlloc&& on_alloc)
{
    const int k = f.k;
    // the oldest frame any transition that stays live references: slot `pos` itself is being replaced
    uint64_t oldest_live = UINT64_MAX;
    const uint64_t live = std::min(pushed, f.capacity);
    if (live > 0) {
        if (pushed < f.capacity) oldest_live = f.first_ref[(pos + f.capacity - live) % f.capacity];
        else if (f.capacity > 1) oldest_live = f.first_ref[(pos + 1) % f.capacity];
    }
    if (f.have_last) oldest_live = std::min(oldest_live, *std::min_element(f.last_next_seq.begin(), f.last_next_seq.end()));
    auto alloc = [&](int src, int j, uint64_t limit, uint64_t* seq) -> bool {
        if (f.frame_seq >= f.frame_cap && f.frame_seq - f.frame_cap >= limit) return false;   // would overwrite a live frame
        on_alloc(src, j, f.frame_seq);
        *seq = f.frame_seq++;
        return true;
    };
    auto all = [&](int q0, int n) { for (int j = 0; j < n; ++j) if (!eq(q0 + j)) return false; return true; };
    std::vector<uint64_t>& oseq = f.oseq; std::vector<uint64_t>& nseq = f.nseq;
    if (f.have_last && all(frame_q_P(k, 0), k)) oseq = f.last_next_seq;
    else {
        for (int j = k - 1; j >= 0; --j) {   // oldest first, so that sequence numbers grow with time
            if (j < k - 1 && eq(frame_q_A(k, j))) oseq[j] = oseq[j + 1];
            else if (!alloc(0, j, oldest_live, &oseq[j])) return false;
        }
    }
    const uint64_t limit = std::min(oldest_live, *std::min_element(oseq.begin(), oseq.end()));
    if (k > 1 && all(frame_q_S(k, 0), k - 1)) {
        for (int j = 1; j < k; ++j) nseq[j] = oseq[j - 1];
        if (eq(frame_q_N(k, 0))) nseq[0] = nseq[1];
        else if (!alloc(1, 0, limit, &nseq[0])) return false;
    } else {
        for (int j = k - 1; j >= 0; --j) {
            if (j < k - 1 && eq(frame_q_N(k, j))) nseq[j] = nseq[j + 1];
            else if (!alloc(1, j, limit, &nseq[j])) return false;
        }
    }
    uint64_t fr = UINT64_MAX;
    for (int j = 0; j < k; ++j) fr = std::min(fr, std::min(oseq[j], nseq[j]));
    f.first_ref[pos] = fr;
    f.last_next_seq = nseq; f.have_last = true;
    return true;
}

}  // namespace bdr
