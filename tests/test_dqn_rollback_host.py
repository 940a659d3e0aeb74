"""Step counters of the DQN agent after a gate time-out (border_amd/csrc/dqn_rollback.hpp), on the host alone.

The fused update applies its optimizer step in three passes - l1 / l2, conv1, conv2 + conv3 - and each records on the device the
step number it applied unless the poison word was up.  After a time-out the host's counters go back to what the device holds:
adam_step to the l1 / l2 word, and each conv segment continues from the step number its moments are at (adam_step - lag).  The
header has no HIP in it: it is compiled here with the host compiler into a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "dqn_rollback.hpp"
// argv: applied0 applied1 applied2 adam_step lag0 lag1 n_opts soft_update_counter n_updates_per_opt soft_update_interval
static void show(const bdr::DqnRollback& r)
{
    printf("%d %llu %llu %lld %lld %llu %llu\n", r.changed ? 1 : 0, (unsigned long long)r.skipped, (unsigned long long)r.c.adam_step, (long long)r.c.lag[0],
           (long long)r.c.lag[1], (unsigned long long)r.c.n_opts, (unsigned long long)r.c.soft_update_counter);
}
int main(int argc, char** argv)
{
    if (argc != 11) return 2;
    const unsigned long long applied[3] = {strtoull(argv[1], 0, 10), strtoull(argv[2], 0, 10), strtoull(argv[3], 0, 10)};
    bdr::DqnStepCounters c{strtoull(argv[4], 0, 10), {atoll(argv[5]), atoll(argv[6])}, strtoull(argv[7], 0, 10), strtoull(argv[8], 0, 10)};
    const uint64_t nupo = strtoull(argv[9], 0, 10), iv = strtoull(argv[10], 0, 10);
    const bdr::DqnRollback first = bdr::dqn_rollback(applied, c, nupo, iv);
    show(first);
    show(bdr::dqn_rollback(applied, first.c, nupo, iv));   // the same device words again
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("rollback")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "rollback"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "border_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def roll(prog, applied, adam_step, lags, n_opts, suc, nupo, iv):
    out = subprocess.run([prog, *map(str, [*applied, adam_step, *lags, n_opts, suc, nupo, iv])], capture_output=True, text=True, check=True).stdout.split("\n")
    first, second = [list(map(int, line.split())) for line in out[:2]]
    keys = ("changed", "skipped", "adam_step", "lag0", "lag1", "n_opts", "suc")
    return dict(zip(keys, first)), dict(zip(keys, second))


# (name, applied words, host counters before (adam_step, lags, n_opts, soft-update counter), n_updates_per_opt, interval,
#  expected after: skipped, adam_step, lags, n_opts, soft-update counter).  The host is at update S = 10 unless said otherwise.
CASES = [
    # every pass of update 10 ran: nothing to take back
    ("all three applied", (10, 10, 10), (10, (0, 0), 10, 10 % 3), 1, 3, (0, 10, (0, 0), 10, 1)),
    # the time-out fell behind the l1 / l2 pass of update 10: both conv segments stay at step 9
    ("l1/l2 only", (10, 9, 9), (10, (0, 0), 10, 1), 1, 3, (0, 10, (1, 1), 10, 1)),
    # ... behind conv1's pass as well: only conv2 + conv3 missed update 10
    ("l1/l2 + conv1", (10, 10, 9), (10, (0, 0), 10, 1), 1, 3, (0, 10, (0, 1), 10, 1)),
    # conv1's pass of update 10 ran on the dX queue BEFORE the weight-gradient queue reached the l1 / l2 pass, which was then
    # skipped with conv2 + conv3: the update is taken back, conv1 is one step ahead of the two other segments
    ("conv1 ahead by one", (9, 10, 9), (10, (0, 0), 10, 1), 1, 3, (1, 9, (-1, 0), 9, 0)),
    # conv2 + conv3 were already one step behind (an earlier time-out), and missed update 10 again: conv1 is two ahead of them
    ("conv1 ahead by two", (10, 10, 8), (10, (0, 1), 10, 1), 1, 3, (0, 10, (0, 2), 10, 1)),
    # the host ran four updates past the last one that was applied
    ("nothing applied across four updates", (6, 6, 6), (10, (0, 0), 10, 1), 1, 3, (4, 6, (0, 0), 6, 0)),
    # ... with two updates per opt: four updates are two opts, interval 5
    ("nothing applied, two updates per opt", (16, 16, 16), (20, (0, 0), 10, 0), 2, 5, (4, 16, (0, 0), 8, 3)),
    # ... with lags from an earlier time-out: they stay what they were (each segment missed the same four updates)
    ("nothing applied, segments already apart", (6, 7, 5), (10, (-1, 1), 10, 1), 1, 3, (4, 6, (-1, 1), 6, 0)),
    # a fresh agent
    ("no update yet", (0, 0, 0), (0, (0, 0), 0, 0), 1, 3, (0, 0, (0, 0), 0, 0)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rollback_returns_to_the_state_the_moments_are_in(prog, case):
    _, applied, (adam_step, lags, n_opts, suc), nupo, iv, want = case
    first, second = roll(prog, applied, adam_step, lags, n_opts, suc, nupo, iv)
    skipped, w_step, w_lags, w_opts, w_suc = want
    assert (first["skipped"], first["adam_step"], (first["lag0"], first["lag1"]), first["n_opts"], first["suc"]) == (skipped, w_step, w_lags, w_opts, w_suc)
    assert first["changed"] == int((w_step, w_lags) != (adam_step, tuple(lags)))
    # every segment's step number is the one its pass last applied (or, never past what the host enqueued, the number it was at)
    assert first["adam_step"] == min(applied[0], adam_step)
    for k in range(2):
        assert first["adam_step"] - first[f"lag{k}"] == min(applied[1 + k], adam_step - lags[k])
    # the same device words a second time: nothing moves
    assert second["changed"] == 0 and second["skipped"] == 0
    assert {k: second[k] for k in ("adam_step", "lag0", "lag1", "n_opts", "suc")} == {k: first[k] for k in ("adam_step", "lag0", "lag1", "n_opts", "suc")}
