"""The model table (border_amd/csrc/param_table.hpp) without a GPU: tools/param_table_sim.cpp - a stand-alone program with its own
main, built with -fsanitize=address,undefined and run directly - drives a fake agent whose arenas are host vectors and whose files
are in-memory buffers through one scenario and prints what happened.  The expectation below is a restatement of the rules:

  an unknown id or a wrong count is refused and changes nothing;   set then get returns the same bits;   a set clears the padding;
  save visits files and their models in the declared order;   load reads EVERY file before it writes any arena (a corrupt last file
  leaves everything as it was) and then applies the files in order, so the later file wins;   params_quiesce runs first, once per
  call, params_written after each arena written, arena_handed_out from arena().

The fake agent: model 0 reference [3][5] <-> arena [8][4] transposed and padded, models 1 and 3 seven values in 8 floats, model 2
one value in 4 floats; files net = models 0 + 2, q = model 1, q.tgt = saved from model 3 and loaded into model 1."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = {0: 15, 1: 7, 2: 1, 3: 7}
FLOATS = {0: 32, 1: 8, 2: 4, 3: 8}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("param_table") / "param_table_sim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "param_table_sim.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", res.stderr     # (a sanitizer report ends the program with a non-zero status)
    return res.stdout.splitlines()


def values(which, generation):
    return np.array([generation * 10000 + which * 100 + i + 0.5 for i in range(COUNT[which])], np.float32)


def arena_of(which, ref):
    """the arena a set leaves behind: padding exactly zero"""
    a = np.zeros(FLOATS[which], np.float32)
    if which == 0:
        a.reshape(8, 4)[:5, :3] = ref.reshape(3, 5).T
    else:
        a[:COUNT[which]] = ref
    return a


def fmt(xs):
    return "".join(" %g" % x for x in xs)


def arenas(state):
    return [f"arena {w}:" + fmt(arena_of(w, state[w])) for w in range(4)]


def expected():
    out = [f"count {w} {COUNT.get(w, 0)}" for w in (-1, 0, 1, 2, 3, 4, 100)]
    state = {}
    for w in range(4):
        state[w] = values(w, 1)
        out += [f"set {w} -> 0", f"trace set_params: quiesce from_host:{w} written:{w}",
                f"get {w} -> 0:" + fmt(state[w]), f"trace get_params: quiesce to_host:{w}"]
    out += arenas(state)
    out += ["error unknown model 4", "set unknown -> 3", "error unknown model -1", "get unknown -> 3",
            "error parameter count mismatch: model 0 holds 15 values, the caller has 14", "set short -> 3",
            "error parameter count mismatch: model 1 holds 7 values, the caller has 8", "get long -> 3",
            "arena unknown -> null 0", "trace refused: quiesce quiesce quiesce quiesce quiesce"]
    out += arenas(state)
    out += ["arena 1 -> model 1 8", "trace arena: quiesce handed_out:1"]
    out += ["save -> 0", "trace save: quiesce to_host:0 to_host:2 write:net to_host:1 write:q to_host:3 write:q.tgt"]
    disk = {"net": np.concatenate([state[0], state[2]]), "q": state[1], "q.tgt": state[3]}
    out += [f"file {k}:" + fmt(disk[k]) for k in sorted(disk)]
    state = {w: values(w, 2) for w in range(4)}
    out += ["load corrupt -> 7", "trace load: quiesce read:net read:q read:q.tgt"]
    out += arenas(state)
    out += ["load -> 0", "trace load: quiesce read:net read:q read:q.tgt from_host:0 written:0 from_host:2 written:2 from_host:1 written:1 "
                         "from_host:1 written:1"]
    state.update({0: disk["net"][:15], 2: disk["net"][15:], 1: disk["q.tgt"]})     # q.tgt is applied after q: the later file wins; model 3 stays
    out += arenas(state)
    return out


def test_the_table_does_what_the_rules_say(lines):
    assert lines == expected()


def test_what_the_scenario_is_there_for(lines):
    """the properties by name, so that a change of the scenario cannot quietly drop one"""
    e = lines.index("error unknown model 4")                                               # the four arenas are printed just before it
    a0 = np.array(lines[e - 4].split()[2:], np.float32)                                    # arena 0 after the sets
    assert a0.size == 32 and (a0.reshape(8, 4)[5:] == 0).all() and (a0.reshape(8, 4)[:, 3] == 0).all() and (a0 != -1).all()
    i, j = lines.index("arena unknown -> null 0"), lines.index("arena 1 -> model 1 8")
    assert j == i + 6 and lines[i + 2:j] == lines[e - 4:e]                                          # refused calls changed no arena
    k = lines.index("load corrupt -> 7")
    assert lines[k + 1].endswith("read:q.tgt") and "from_host" not in lines[k + 1]          # the last file failed, nothing was written
    assert lines[k + 2:k + 6] == arenas({w: values(w, 2) for w in range(4)})
    final = lines[-4:]
    assert final[1] == "arena 1:" + fmt(arena_of(1, values(3, 1))) and final[3] == "arena 3:" + fmt(arena_of(3, values(3, 2)))
