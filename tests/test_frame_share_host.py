"""The sharing rule of the single-frame store as code of its own (border_amd/csrc/frame_share.hpp): the host push answers its
equality questions with memcmp, the device push (bdr_replay_push_device_frames) with flags computed in HBM.  Here the header runs
without a GPU: tools/frame_share_sim.cpp - a stand-alone program with its own main, built with -fsanitize=address,undefined and
run directly - reads stacked rows from a file and prints, per transition, the sequence numbers of its frames, first_ref and the
frames it allocated.  The expectation is a restatement of the rule in Python, written from the comment on push_frames
(csrc/replay.hip):
  obs_t == the previous push's next_obs          -> obs costs nothing
  next_obs_t[1..k) == obs_t[0..k-1)              -> next_obs costs its newest frame only
  equal neighbouring frames inside one stack     -> stored once
  frames are allocated in push order in a ring of frame_cap slots; a slot may only be reused once no live transition (nor the
  last next_obs) references it, otherwise the push fails.
Frame size 16 bytes, k in {1, 2, 4, 8}, small capacities."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = 16


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_share") / "frame_share_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "frame_share_sim.cpp"), "-o", exe])
    return exe


# ------------------------------------------------------------------------------------------------ the rule, restated
class Exhausted(Exception):
    pass


def share_rule(obs, nxt, cap, fcap):
    """obs, nxt: [n, k, FB] u8, frames newest first.  -> (lines as the program prints them, index of the transition the store could
    not hold or None)"""
    n, k = obs.shape[:2]
    state = {"seq": 0}
    live = collections.deque()      # first_ref of the live transitions, oldest first
    last = None                     # (next_obs bytes, their sequence numbers) of the previous push
    lines = []

    def alloc(floor, log, tag):
        # slot seq % fcap holds frame seq - fcap: still referenced if it is not older than every frame in use
        if state["seq"] >= fcap and floor is not None and state["seq"] - fcap >= floor:
            raise Exhausted
        log.append(f"{tag}:{state['seq']}")
        state["seq"] += 1
        return state["seq"] - 1

    def place(stack, floor, log, src):
        seqs = [None] * k
        for j in range(k - 1, -1, -1):     # oldest first
            if j < k - 1 and (stack[j] == stack[j + 1]).all():
                seqs[j] = seqs[j + 1]
            else:
                seqs[j] = alloc(floor, log, f"{src}:{j}")
        return seqs

    for s in range(n):
        staying = list(live)[1:] if len(live) == cap else list(live)     # the transition in this ring slot is being replaced
        in_use = staying + (list(last[1]) if last else [])
        floor = min(in_use) if in_use else None
        log = []
        try:
            if last is not None and (obs[s] == last[0]).all():
                oseq = list(last[1])
            else:
                oseq = place(obs[s], floor, log, "o")
            floor2 = min(oseq) if floor is None else min(floor, min(oseq))
            if k > 1 and (nxt[s][1:] == obs[s][:-1]).all():
                nseq = [None] + oseq[:-1]
                nseq[0] = nseq[1] if (nxt[s][0] == nxt[s][1]).all() else alloc(floor2, log, "n:0")
            else:
                nseq = place(nxt[s], floor2, log, "n")
        except Exhausted:
            lines.append(f"{s} exhausted")
            return lines, s
        if len(live) == cap:
            live.popleft()
        live.append(min(oseq + nseq))
        last = (nxt[s].copy(), nseq)
        lines.append(f"{s} {' '.join(map(str, oseq))} | {' '.join(map(str, nseq))} | {live[-1]} |" + "".join(" " + x for x in log))
    return lines, None


# ------------------------------------------------------------------------------------------------ the cases
class Env:
    """A stack of k frames, newest first; a step shifts a new frame in; after an episode end the stack is k copies of one frame."""

    def __init__(self, rng, k, p_done):
        self.rng, self.k, self.p, self.stack = rng, k, p_done, None

    def frame(self):
        return self.rng.integers(0, 256, FB, dtype=np.uint8)

    def step(self):
        if self.stack is None:
            self.stack = np.stack([self.frame()] * self.k)
        o = self.stack.copy()
        self.stack = np.concatenate([self.frame()[None], self.stack[:-1]])
        x = self.stack.copy()
        if self.rng.random() < self.p:
            self.stack = None
        return o, x


def make_case(name, k, rng):
    """-> obs, next_obs, capacity, frame_capacity"""
    if name == "continuing":          # one episode, the ring does not fill
        e = Env(rng, k, 0.0)
        tr, cap, fcap = [e.step() for _ in range(12)], 16, 16 + 16 // 4 + 64
    elif name == "resets":            # reset stacks: all k frames equal
        e = Env(rng, k, 0.3)
        tr, cap, fcap = [e.step() for _ in range(24)], 32, 32 + 32 // 4 + 64
    elif name == "interleaved":       # two environments take turns: obs never continues the previous push
        es = [Env(rng, k, 0.1), Env(rng, k, 0.1)]
        tr, cap, fcap = [es[t % 2].step() for t in range(20)], 32, 32 * (k + 1) + 64
    elif name == "wrapping":          # transition ring (5 slots) and frame ring wrap several times
        e = Env(rng, k, 0.15)
        cap, fcap = 5, 2 * 5 + 4 * k + 3
        tr = [e.step() for _ in range(3 * fcap)]
    elif name == "exhausted":         # rows that share nothing: 2k frames per transition into a store that is too small
        tr = [(rng.integers(0, 256, (k, FB), dtype=np.uint8), rng.integers(0, 256, (k, FB), dtype=np.uint8)) for _ in range(12)]
        cap, fcap = 8, 2 * k * 5 + 1
    obs, nxt = np.stack([t[0] for t in tr]), np.stack([t[1] for t in tr])
    return obs, nxt, cap, fcap


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("case", ["continuing", "resets", "interleaved", "wrapping", "exhausted"])
def test_the_header_gives_every_transition_what_the_rule_says(sim, tmp_path, case, k):
    rng = np.random.default_rng(100 * k + len(case))
    obs, nxt, cap, fcap = make_case(case, k, rng)
    n = len(obs)
    path = tmp_path / "rows.bin"
    np.concatenate([obs.reshape(n, -1), nxt.reshape(n, -1)], axis=1).tofile(path)
    res = subprocess.run([sim, str(k), str(FB), str(cap), str(fcap), str(n), str(path)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr     # (a sanitizer report ends the program with a non-zero status)
    want, failed_at = share_rule(obs, nxt, cap, fcap)
    got = [" ".join(l.split()) for l in res.stdout.splitlines()]
    assert got == [" ".join(l.split()) for l in want]
    # what each case is there for
    used = 1 + max(int(x.rsplit(":", 1)[1]) for l in got for x in l.split() if re.fullmatch(r"[on]:\d+:\d+", x))
    if case == "exhausted":
        assert failed_at is not None and 0 < failed_at < n and got[-1] == f"{failed_at} exhausted"
    else:
        assert failed_at is None and len(got) == n
    if case == "continuing":
        assert used == n + 1                       # the reset stack once, then one frame per transition
    if case == "resets" and k > 1:
        assert any(len(set(l.split("|")[0].split()[1:])) == 1 for l in got[1:])      # a reset stack after the first: one frame
    if case == "interleaved" and k > 1:
        assert used > 2 * n                        # no obs continues the push before it: obs is stored again
    if case == "wrapping":
        assert used > 2 * fcap and n > 2 * cap


def test_the_new_call_is_on_every_surface():
    from border_amd import _lib, build
    name = "bdr_replay_push_device_frames"
    assert hasattr(C.CDLL(build.build_library()), name)
    assert name in _lib.ABI_SYMBOLS
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    assert re.search(rf"pub fn {name}\s*\(", ffi)
    assert f"ffi::{name}(" in open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "replay.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    assert re.search(rf"BDR_API int32_t {name}\(", hdr)
    from border_amd import SimpleReplayBuffer
    assert callable(SimpleReplayBuffer.push_device_frames)
