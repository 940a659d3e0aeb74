"""The staging-slot rule of the agent group (border_amd/csrc/slot_ring.hpp), on the host alone.

Three rings - per-step words, prioritized-replay words, push records - take their slots in turn by their own use count and draw
launch numbers from ONE counter; a slot is rewritten once the pinned sequence word has reached the number recorded for it.  The
header has no HIP in it: it is compiled here with the host compiler into a program of its own, which drives the three rings through
the interleavings the group produces against a model of the device: a published number that trails the counter by an arbitrary lag.
The program checks, at every use of a slot:
  (a) the wait target handed out equals the highest launch number that ever read the slot (kept by the model, not by the ring), and
      once the 32-bit word has reached it every such launch really is through;
  (b) for the step ring the target is never later than launch k - DEPTH, the rule "slot k mod DEPTH, wait for launch k - DEPTH"
      that the ring replaces (k: the number of the launch being prepared);
  (c) DEPTH consecutive uses name DEPTH distinct slots;
  (d) a reset forgets every reader;
and naming a slot without recording a launch leaves the ring where it was.  With the counter started at 2^32 - 5 the sequence word
wraps in the middle of the run (e)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "slot_ring.hpp"

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "line %d: %s: ", __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static unsigned long long rng_state = 1;
static unsigned rnd(unsigned n) { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(rng_state >> 33) % n; }

template <int D> struct Sim {
    struct Tracked {
        bdr::SlotRing<D> ring;
        uint64_t readers[D] = {};          // the model: per slot, the highest launch number that ever read it
        std::vector<int> slots;            // every slot taken, in order
        int taken = -1;
    };
    Tracked step, per, push;
    uint64_t launches, done;               // numbers given out; every launch <= done is through, the word holds (unsigned)done
    uint64_t waits = 0;
    explicit Sim(uint64_t start) : launches(start), done(start) {}

    void device_runs() { if (rnd(4) == 0) done += rnd((unsigned)(launches - done) + 1); }   // an arbitrary lag: now and then, any part of the backlog
    // the host side of group_wait_seq: spin on the 32-bit word
    void wait(uint64_t target)
    {
        if (!target) return;
        while (!bdr::seq_reached((unsigned)done, (unsigned)target)) {
            CHECK(done < launches, "waiting for launch %llu, which was never given out (%llu)", (unsigned long long)target, (unsigned long long)launches);
            done += 1; waits += 1;
        }
        CHECK(done >= target, "the word %u counts as having reached %u, but launch %llu is not through (done %llu)", (unsigned)done, (unsigned)target,
              (unsigned long long)target, (unsigned long long)done);
    }
    // take the next slot of `t` for the launch numbered k: (a), and (b) where asked
    void take(Tracked& t, uint64_t k, bool is_step_ring)
    {
        const auto again = t.ring.next(), n = t.ring.next();
        CHECK(again.slot == n.slot && again.wait == n.wait, "naming a slot moved the ring");
        CHECK(n.slot >= 0 && n.slot < D, "slot %d", n.slot);
        CHECK(n.wait == t.readers[n.slot], "(a) slot %d: wait target %llu, last reader %llu", n.slot, (unsigned long long)n.wait, (unsigned long long)t.readers[n.slot]);
        if (is_step_ring && n.wait) CHECK(n.wait + D <= k, "(b) launch %llu: target %llu is later than launch k - %d", (unsigned long long)k, (unsigned long long)n.wait, D);
        wait(n.wait);
        CHECK(t.readers[n.slot] <= done, "slot %d is rewritten while launch %llu may still read it", n.slot, (unsigned long long)t.readers[n.slot]);
        t.taken = n.slot;
    }
    void record(Tracked& t, uint64_t number)
    {
        t.ring.record(number);
        if (number > t.readers[t.taken]) t.readers[t.taken] = number;
        t.slots.push_back(t.taken);
        const size_t n = t.slots.size();
        if (n >= (size_t)D)   // (c)
            for (size_t i = n - D; i < n; ++i) for (size_t j = i + 1; j < n; ++j) CHECK(t.slots[i] != t.slots[j], "(c) uses %zu and %zu share slot %d", i, j, t.slots[i]);
    }
    // the four calls of the group
    void plain_step() { const uint64_t k = launches + 1; take(step, k, true); record(step, k); launches = k; }
    void plain_push() { const uint64_t k = launches + 1; take(push, k, false); record(push, k); launches = k; }
    void per_round()   // the step publishes k, the last tree kernel behind it k + 1
    {
        const uint64_t k = launches + 1;
        take(step, k, true); take(per, k, false);
        record(step, k); record(per, k + 1);
        launches = k + 1;
    }
    void per_push() { const uint64_t k = launches + 1; take(push, k, false); record(push, k + 1); launches = k + 1; }
    void push_realloc()   // behind a stream synchronise
    {
        done = launches;
        push.ring.reset();
        for (int s = 0; s < D; ++s) { CHECK(push.ring.reader[s] == 0, "(d) slot %d still has a reader", s); push.readers[s] = 0; }
        CHECK(push.ring.next().wait == 0, "(d) a wait target after the reset");
        push.slots.clear();
    }
};

template <int D> int run(int mode, uint64_t start, int iters)
{
    Sim<D> s(start);
    for (int it = 0; it < iters; ++it) {
        switch (mode) {
        case 0: s.plain_step(); break;
        case 1: s.plain_push(); s.device_runs(); s.plain_step(); break;
        case 2: s.per_round(); s.device_runs(); s.per_push(); break;
        default:
            switch (rnd(9)) {
            case 0: case 1: s.plain_step(); break;
            case 2: case 3: s.plain_push(); break;
            case 4: case 5: s.per_round(); break;
            case 6: case 7: s.per_push(); break;
            default: s.push_realloc(); break;
            }
        }
        s.device_runs();
    }
    if (mode != 3) { s.push_realloc(); s.plain_push(); }
    if (start) CHECK((unsigned)s.launches < (unsigned)start, "the sequence word did not wrap");
    printf("%llu %llu %zu %zu %zu\n", (unsigned long long)(s.launches - start), (unsigned long long)s.waits, s.step.slots.size(), s.per.slots.size(), s.push.slots.size());
    return 0;
}

// argv: depth mode start iterations seed
int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    CHECK(bdr::seq_reached(5u, 5u) && bdr::seq_reached(6u, 5u) && !bdr::seq_reached(4u, 5u), "seq_reached, no wrap");
    CHECK(bdr::seq_reached(2u, 0xfffffffeu) && !bdr::seq_reached(0xfffffffeu, 2u) && bdr::seq_reached(0u, 0xffffffffu), "seq_reached across the wrap");
    CHECK(bdr::seq_reached(0x7fffffffu, 1u) && !bdr::seq_reached(0x80000001u, 1u), "seq_reached, 2^31 - 2 and 2^31 apart");
    const int depth = atoi(argv[1]), mode = atoi(argv[2]), iters = atoi(argv[4]);
    const uint64_t start = strtoull(argv[3], 0, 10);
    rng_state = strtoull(argv[5], 0, 10);
    if (depth == 8) return run<8>(mode, start, iters);
    if (depth == 2) return run<2>(mode, start, iters);
    return 2;
}
"""

MODES = ("steps only", "push and step alternating", "prioritized rounds and prioritized pushes alternating", "a mix of all")
ITERS = 300


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("slot_ring")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "slot_ring"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("start", [0, 2**32 - 5], ids=["from 0", "word wraps"])
@pytest.mark.parametrize("mode", range(4), ids=MODES)
@pytest.mark.parametrize("depth", [8, 2])
def test_every_slot_waits_for_its_last_reader(prog, depth, mode, start):
    for seed in (1, 2, 3):
        r = subprocess.run([prog, str(depth), str(mode), str(start), str(ITERS), str(seed)], capture_output=True, text=True)
        assert r.returncode == 0, (seed, r.stderr)
        launches, waits, n_step, n_per, n_push = map(int, r.stdout.split())
        # the run did what its name says: every ring it drives was used well past its depth, and the host did have to wait
        if mode == 0: assert (launches, n_step, n_per) == (ITERS + 1, ITERS, 0)
        if mode == 1: assert (launches, n_step, n_per) == (2 * ITERS + 1, ITERS, 0)
        if mode == 2: assert (launches, n_step, n_per) == (4 * ITERS + 1, ITERS, ITERS)
        if mode == 3: assert min(n_step, n_per) > 4 * depth and launches > ITERS
        assert waits > 0
