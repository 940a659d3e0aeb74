// Reuse of pinned staging slots that kernels read in place (the agent group's per-step words, prioritized-replay words and push
// records; agent_group.hpp).  No HIP in here: the bookkeeping is tested on its own with the host compiler (tests/test_slot_ring_host.py).
//
// A pinned slot is read when the kernel runs, not when it is enqueued, so the host may rewrite it only after the last launch that
// reads it is through.  Every launch of an owner takes a number from ONE counter (1, 2, ...) and publishes it, truncated to 32 bits,
// to ONE pinned word when it ends; where more kernels read the slot behind it, the last of them publishes the next number for it.
// The launches run on one stream, so "number n has been published" means every launch numbered <= n is through.
//
// The one rule, for every ring: it takes its slots in turn BY ITS OWN USE COUNT, remembers per slot the number of the last launch
// that read it and hands that number out with the slot; the host writes the slot once the word has reached it (0: never read).  The
// use count moves only when a launch is recorded: a call that fails between taking a slot and launching leaves the ring as it was.
//
// Several rings may share the counter.  A ring of depth D then never waits longer than the rule "slot k mod D for launch k, wait for
// launch k - D" would: the launch recorded for a slot lies D uses of this ring back, every use took at least one number, and a use
// recorded with the number after its own (k' + 1) took both - so with k the next number given out, recorded <= k - D.  That rule is
// safe too (every earlier reader of slot k mod D has a number <= k - D), but with other launches drawing numbers in between it
// leaves slots unused and waits for launches that never read the slot; this one uses all D slots and waits for the slot's reader.
#pragma once
#include <cstdint>

namespace bdr {

// has the 32-bit sequence word `done` reached `seq`?  Wrap-safe while the two are less than 2^31 launches apart.
inline bool seq_reached(unsigned done, unsigned seq) { return (int)(done - seq) >= 0; }

template <int DEPTH>
struct SlotRing {
    static_assert(DEPTH >= 1, "a ring has at least one slot");
    struct Next { int slot; uint64_t wait; };   // wait: the launch number that must have been published before `slot` is rewritten (0: none)
    uint64_t uses = 0;                          // launches recorded so far
    uint64_t reader[DEPTH] = {};                // per slot: the number of the last launch that read it (0: never read)

    Next next() const { const int s = (int)(uses % DEPTH); return Next{s, reader[s]}; }
    // the launch that reads the slot next() named (or the last kernel behind it that does) carries number `launch`
    void record(uint64_t launch) { reader[uses % DEPTH] = launch; uses += 1; }
    // the slots were reallocated behind a stream synchronise: nothing reads them any more
    void reset() { *this = SlotRing(); }
};

}  // namespace bdr
