// Host-side step counters of the DQN agent after a gate time-out (DqnCnn::on_gate_timeout).  No HIP in here: the arithmetic is
// tested on its own with the host compiler (tests/test_dqn_rollback_host.py).
//
// The fused update applies its optimizer step in three passes, each of which records the step number it applied in its own device
// word unless the poison word was up (then it is skipped):
//   [0] l1 / l2              k_adam on the weight-gradient queue (or the whole-arena pass of adam_all)
//   [1] conv1                k_reduce_adam{conv1} on the dX queue
//   [2] conv2 + conv3        k_reduce_adam{conv2, conv3} on the weight-gradient queue (schedules without the overlapped tail: one
//                            launch for [1] and [2])
// The host counts one step per update (adam_step, the l1 / l2 segment's number); a conv segment's number is adam_step - lag[k].
// After a time-out the host's numbers go back to what the device applied: adam_step to applied[0], and every conv segment continues
// from the step number ITS moments are at - a time-out that fell between the passes of one update leaves a segment one step
// behind (lag 1) or, where its pass ran before the l1 / l2 pass that was skipped, one ahead (lag -1).  n_opts and the soft-update
// counter follow the l1 / l2 segment (k_track is poison-gated like the optimizer passes).
#pragma once
#include <algorithm>
#include <cstdint>

namespace bdr {

struct DqnStepCounters {
    uint64_t adam_step;             // optimizer steps of the l1 / l2 segment = updates counted by the host
    int64_t lag[2];                 // conv1, conv2 + conv3: the segment's step number is adam_step - lag
    uint64_t n_opts;
    uint64_t soft_update_counter;
};

struct DqnRollback {
    DqnStepCounters c;              // the counters to continue with
    uint64_t skipped;               // updates taken back (0: nothing to roll back, c is the input)
    bool changed;
};

inline DqnRollback dqn_rollback(const unsigned long long (&applied)[3], const DqnStepCounters& in, uint64_t n_updates_per_opt, uint64_t soft_update_interval)
{
    DqnRollback r{in, 0, false};
    int64_t now[2];
    bool behind = applied[0] < in.adam_step;
    for (int k = 0; k < 2; ++k) {
        now[k] = (int64_t)in.adam_step - in.lag[k];
        behind = behind || (int64_t)applied[1 + k] < now[k];
    }
    if (!behind) return r;
    r.changed = true;
    r.skipped = in.adam_step - std::min<uint64_t>(applied[0], in.adam_step);
    r.c.adam_step = in.adam_step - r.skipped;
    for (int k = 0; k < 2; ++k) {
        const uint64_t at = std::min<uint64_t>(applied[1 + k], (uint64_t)std::max<int64_t>(now[k], 0));   // (never past what the host has enqueued)
        r.c.lag[k] = (int64_t)r.c.adam_step - (int64_t)at;
    }
    const uint64_t opts_back = std::min(in.n_opts, r.skipped / std::max<uint64_t>(1, n_updates_per_opt));
    r.c.n_opts = in.n_opts - opts_back;
    // the soft updates of the skipped opts were skipped on the device with them: their counter goes back too
    const uint64_t iv = std::max<uint64_t>(1, soft_update_interval);
    r.c.soft_update_counter = (in.soft_update_counter + iv - opts_back % iv) % iv;
    return r;
}

}  // namespace bdr
