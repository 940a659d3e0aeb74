"""Prioritized replay under an agent group (bdr_agent_group_set_prioritized, DqnGroup(prioritized=True)) against its TWINS: standalone
agents with the same configs and seeds on prioritized rings fed the same pushes, stepped one after the other.  Equality is `==` on
every element: arenas, losses, n_opts, each ring's whole f32 sum tree, per_info (n_samples, PER n_opts, beta, total, min, max), the
last batch's indices, weights and rows, ring rows, head, size and the index stream."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_agent_group import ARENAS, Ring, assert_same, cfg, clean_env, hetero, state
from tests.test_gpu_group_push import assert_same_ring, draw, group_push, ring_state, row

pytestmark = pytest.mark.gpu

# the issue's table: capacity, alpha, normaliser of the five `hetero` members' rings (n_opts_final = 10: beta reaches beta_final in the run)
PER = [(700, 0.6, "All"), (37, 1.0, "Batch"), (1000, 0.6, "Batch"), (5000, 0.6, "All"), (8, 1.0, "All")]


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


class PRing(Ring):
    """Ring of tests/test_gpu_agent_group.py on a prioritized buffer (per=None: the uniform ring it is there)"""
    def __init__(self, B, c, seed, per, first=None):
        q = c.model_config.q_config
        self.in_dim, self.A = q.in_dim, q.out_dim
        self.rng = np.random.default_rng(1000 + seed)
        capacity, pc = 700, None
        if per is not None:
            capacity = per[0]
            pc = B.PerConfig(alpha=per[1], n_opts_final=10, normalize=per[2])
        self.per = per is not None
        self.rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed, per_config=pc), (self.in_dim,), np.float32)
        first = min(300, capacity - 3) if first is None else first   # (the small rings start part filled and wrap with the first pushes)
        if first: self.push(first)


def last_batch(rb, n):
    """indices, weights, obs rows and rewards of the batch drawn last (device arrays of bdr_replay_last_batch)"""
    from border_amd import _lib
    db = _lib.DeviceBatch()
    _lib.check(_lib.lib().bdr_replay_last_batch(rb.handle, C.byref(db)))
    assert db.n == n
    hip = C.CDLL("libamdhip64.so")
    def fetch(ptr, shape, dtype):
        out = np.empty(shape, dtype)
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
        return out
    w = np.empty(n, np.float32)
    _lib.check(_lib.lib().bdr_replay_batch_weights(rb.handle, n, w.ctypes.data_as(C.c_void_p)))
    return {"ixs": fetch(db.ixs, n, np.uint64), "w": w, "obs": fetch(db.obs, (n,) + tuple(rb.obs_shape), np.float32),
            "reward": fetch(db.reward, n, np.float32)}


def pstate(agent, ring, losses):
    agent.sync()
    out = {"arenas": {k: agent.get_params(k) for k in ARENAS}, "losses": losses, "n_opts": agent.n_opts}
    if ring.per:
        out["batch"] = last_batch(ring.rb, agent.config.batch_size)
        out["tree"] = ring.rb.per_tree()
        out["info"] = ring.rb.per_info()
    out["ring"] = ring_state(ring.rb)   # rows, len, head, summary and 40 draws of the index stream
    s = out["ring"]["summary"]
    out["ring"]["summary"] = (s[0], s[1], np.float32(s[2]).tobytes())   # (the reward sum by its bits: one test's is NaN)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_psame(got, want, what="", finite=True):
    for k in ARENAS:
        assert (bits(got["arenas"][k]) == bits(want["arenas"][k])).all(), (what, k)
    if finite: assert np.isfinite(got["arenas"]["qnet"]).all(), what
    assert np.array(got["losses"], np.float32).tobytes() == np.array(want["losses"], np.float32).tobytes(), (what, "losses")
    assert got["n_opts"] == want["n_opts"], (what, "n_opts")
    assert ("tree" in got) == ("tree" in want)
    if "tree" in want:
        assert got["tree"].shape == want["tree"].shape and (bits(got["tree"]) == bits(want["tree"])).all(), (what, "sum tree")
        assert got["info"] == want["info"], (what, got["info"], want["info"])
        for k in ("ixs", "w", "obs", "reward"):
            assert (bits(got["batch"][k]) == bits(want["batch"][k])).all(), (what, "last batch", k)
    assert_same_ring(got["ring"], want["ring"], what)


def run_twins(B, members, pers, schedule):
    """schedule(step(record, only=None), push(n), ring_call(i, fn)) for one twin at a time"""
    out = []
    for i, ((c, seed), per) in enumerate(zip(members, pers)):
        a, ring = B.Dqn.build(c), PRing(B, c, seed, per)
        losses = []
        def step(record, only=None):
            if only not in (None, i): return
            if record: losses.append(a.opt_with_record(ring.rb)["loss"])
            else: a.opt(ring.rb)
        schedule(step, lambda n: ring.push(n), lambda j, fn: fn(ring.rb, a) if j == i else None)
        out.append(pstate(a, ring, losses))
        a.close(); ring.rb.close()
    return out


def run_group(B, members, pers, schedule, prioritized=True):
    g = B.DqnGroup.build([c for c, _ in members], prioritized=prioritized)
    assert g.prioritized == prioritized
    rings = [PRing(B, c, seed, per) for (c, seed), per in zip(members, pers)]
    bufs = [r.rb for r in rings]
    losses = [[] for _ in members]
    def step(record, only=None):
        if only is not None:
            m = g.members[only]
            if record: losses[only].append(m.opt_with_record(bufs[only])["loss"])
            else: m.opt(bufs[only])
        elif record:
            for l, rec in zip(losses, g.opt_with_record(bufs)): l.append(rec["loss"])
        else:
            g.opt(bufs)
    def push(n):
        for r in rings: r.push(n)
    schedule(step, push, lambda j, fn: fn(bufs[j], g.members[j]))
    g.sync()
    out = [pstate(m, r, l) for m, r, l in zip(g.members, rings, losses)]
    g.close()
    for r in rings: r.rb.close()
    return out


def twelve_opts(step, push, ring_call):
    for k in range(12):
        step(k % 3 == 0)   # every third opt is opt_with_record
        push(50)


_twins = {}


def twins_of_case1(B, n_upd):
    if n_upd not in _twins:
        _twins[n_upd] = run_twins(B, hetero(B, n_upd), PER, twelve_opts)
    return _twins[n_upd]


@pytest.mark.parametrize("n_upd", [1, 2])
def test_heterogeneous_prioritized_group_equals_its_twins(B, n_upd, monkeypatch):
    """the five members of tests/test_gpu_agent_group.py on the five rings of PER: both normalisers, alpha 1 and 0.6, a tree past the
    staged top (capacity 5000), rings smaller than the batch (37 < 64, 8 < 32: every batch has duplicates)"""
    clean_env(monkeypatch)
    want = twins_of_case1(B, n_upd)
    got = run_group(B, hetero(B, n_upd), PER, twelve_opts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_psame(g, w, f"member {i}")
        assert len(g["losses"]) == 4 and g["n_opts"] == 12
        assert g["info"]["n_opts"] == 12 * n_upd and g["info"]["beta"] == 1.0
        assert g["info"]["n_samples"] == min(PER[i][0], min(300, PER[i][0] - 3) + 600)
    assert len(set(got[4]["batch"]["ixs"].tolist())) <= 8 < 32


def test_global_memory_form_same_bits(B, monkeypatch):
    """BDR_NO_MLP_LDS=1: the group entry of k_dqn_mlp_step with weight / td_abs set, against the twins stepped WITHOUT it"""
    clean_env(monkeypatch)
    want = twins_of_case1(B, 1)
    monkeypatch.setenv("BDR_NO_MLP_LDS", "1")
    got = run_group(B, hetero(B, 1), PER, twelve_opts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_psame(g, w, f"member {i}")


def test_mixed_group_and_calls_of_the_members_own(B, monkeypatch):
    """members 0 and 2 prioritized, 1 and 3 uniform; member 2 alone through its own opt, rb.batch and rb.update_priority directly on
    member 0's ring, all between group opts"""
    clean_env(monkeypatch)
    members = hetero(B, 1)[:4]
    pers = [PER[0], None, PER[2], None]
    def own_calls(rb, agent):
        b = rb.batch(16)
        rb.update_priority(b.ix_sample, np.linspace(0.1, 2.0, 16).astype(np.float32))
    def sched(step, push, ring_call):
        step(False); push(20)
        step(False, only=2); step(True, only=2)
        ring_call(0, own_calls)
        push(20); step(True)
        ring_call(0, own_calls)
        step(False)
    want = run_twins(B, members, pers, sched)
    got = run_group(B, members, pers, sched)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_psame(g, w, f"member {i}")
    assert [g["n_opts"] for g in got] == [3, 3, 5, 3]
    assert [("tree" in g) for g in got] == [True, False, True, False]
    assert got[0]["info"]["n_opts"] == 5 and got[2]["info"]["n_opts"] == 5


def test_grouped_push_on_prioritized_rings(B, monkeypatch):
    """40 grouped pushes back to back (every staging slot rewritten five times) into EMPTY prioritized rings of capacity 5 (wraps eight
    times: the maximum leaf is overwritten), 700 and 64, a group opt after the 25th - against rb.push of one row and a.opt"""
    clean_env(monkeypatch)
    assert 40 >= 4 * B.DqnGroup.PUSH_STAGING_DEPTH
    h = hetero(B, 1)
    members = [h[0], h[1], h[4]]
    pers = [(5, 1.0, "All"), (700, 0.6, "Batch"), (64, 0.6, "All")]
    cols = [draw(np.random.default_rng(90 + i), 4, 2, 40) for i in range(3)]
    want = []
    for i, ((c, seed), per) in enumerate(zip(members, pers)):
        a, ring = B.Dqn.build(c), PRing(B, c, seed, per, first=0)
        for k in range(40):
            ring.rb.push(*row(cols[i], k))
            if k == 24: a.opt(ring.rb)
        want.append(pstate(a, ring, []))
        a.close(); ring.rb.close()
    g = B.DqnGroup.build([c for c, _ in members], prioritized=True)
    rings = [PRing(B, c, seed, per, first=0) for (c, seed), per in zip(members, pers)]
    bufs = [r.rb for r in rings]
    for k in range(40):
        group_push(g, cols, k, bufs if k == 0 else None, as_array=True)
        if k == 24: g.opt(bufs)
    g.sync()
    for i, (m, r) in enumerate(zip(g.members, rings)):
        got = pstate(m, r, [])
        assert_psame(got, want[i], f"member {i}")
        assert got["ring"]["len"] == min(40, pers[i][0]) and got["ring"]["head"] == 40 % pers[i][0]
        assert got["info"]["n_samples"] == min(40, pers[i][0]) and got["info"]["n_opts"] == 1
    g.close()
    for r in rings: r.rb.close()


def test_push_and_opt_alternating_on_prioritized_rings(B, monkeypatch):
    """40 iterations of (one grouped push of one row, one group opt), no synchronise and no acting call in between, on prioritized rings
    of capacity 5, 33 and 33 that start part filled and wrap: the step words, the prioritized words and the push records each go round
    their staging ring five times by their own use count, every round and every push taking two launch numbers of the one counter"""
    clean_env(monkeypatch)
    assert 40 >= 4 * max(B.DqnGroup.STAGING_DEPTH, B.DqnGroup.PUSH_STAGING_DEPTH)
    members = hetero(B, 1)[:3]
    pers = [(5, 1.0, "All"), (33, 0.6, "Batch"), (33, 0.6, "All")]
    want = []
    for (c, seed), per in zip(members, pers):
        a, ring = B.Dqn.build(c), PRing(B, c, seed, per)
        cols = draw(ring.rng, ring.in_dim, ring.A, 40)
        for k in range(40):
            ring.rb.push(*row(cols, k))
            a.opt(ring.rb)
        want.append(pstate(a, ring, []))
        a.close(); ring.rb.close()
    g = B.DqnGroup.build([c for c, _ in members], prioritized=True)
    rings = [PRing(B, c, seed, per) for (c, seed), per in zip(members, pers)]
    bufs = [r.rb for r in rings]
    cols = [draw(r.rng, r.in_dim, r.A, 40) for r in rings]
    for k in range(40):
        group_push(g, cols, k, bufs)
        g.opt(bufs)
    g.sync()
    for i, (m, r) in enumerate(zip(g.members, rings)):
        got = pstate(m, r, [])
        assert_psame(got, want[i], f"member {i}")
        assert got["n_opts"] == 40 and got["info"]["n_opts"] == 40 and got["info"]["n_samples"] == pers[i][0]
        assert got["ring"]["len"] == pers[i][0] and got["ring"]["head"] == (pers[i][0] - 3 + 40) % pers[i][0]
    g.close()
    for r in rings: r.rb.close()


def test_group_loop_on_prioritized_rings_equals_three_single_loops(B, monkeypatch):
    """DqnGroup.train over three members on prioritized rings against three Trainer runs on twins"""
    from border_amd.trainer import NativeTrainer, TrainerConfig
    from tests.test_gpu_group_trainer import CONFIG, ToyEnv, prepare
    clean_env(monkeypatch)
    h = hetero(B, 1)
    members = [h[0], h[2], h[3]]
    pers = [(64, 0.6, "All"), (64, 1.0, "Batch"), (64, 0.6, "Batch")]
    dims = [c.model_config.q_config.in_dim for c, _ in members]
    def fin(agent, ring, events, stats):
        out = pstate(agent, ring, [])
        out["events"] = events
        out["stats"] = {k: stats[k] for k in ("env_steps", "opt_steps", "n_records", "n_episodes")}
        return out
    want = []
    for i, ((c, seed), per) in enumerate(zip(members, pers)):
        a, ring = B.Dqn.build(c), PRing(B, c, seed, per, first=0)
        prepare(B, i, a)
        ev = []
        st = NativeTrainer(TrainerConfig(**CONFIG)).train(ToyEnv(dims[i], 300 + i), a, ring.rb, (dims[i],), np.float32,
                                                          on_event=lambda e, o, name, sc: ev.append((e, o, name, sc)))
        want.append(fin(a, ring, ev, st))
        a.close(); ring.rb.close()
    g = B.DqnGroup.build([c for c, _ in members], prioritized=True)
    for i, m in enumerate(g.members): prepare(B, i, m)
    rings = [PRing(B, c, seed, per, first=0) for (c, seed), per in zip(members, pers)]
    events = [[] for _ in members]
    stats = g.train([ToyEnv(d, 300 + i) for i, d in enumerate(dims)], [r.rb for r in rings], TrainerConfig(**CONFIG),
                    on_event=lambda m, e, o, name, sc: events[m].append((e, o, name, sc)))
    g.sync()
    for i, (m, r) in enumerate(zip(g.members, rings)):
        got = fin(m, r, events[i], stats[i])
        assert_psame(got, want[i], f"member {i}")
        assert got["stats"] == want[i]["stats"] and got["events"] == want[i]["events"], i
        assert got["n_opts"] == 30 and got["info"]["n_opts"] == 30 and got["info"]["n_samples"] == 64
    g.close()
    for r in rings: r.rb.close()


def three_opts(step, push, ring_call):
    step(False); push(30); step(True); step(False)


def test_the_switch(B, monkeypatch):
    """switched on over uniform rings: the default group's bits; the other refusals stay, with nothing advanced; switched off again a
    prioritized ring is refused as before"""
    from border_amd import _lib
    clean_env(monkeypatch)
    members = hetero(B, 1)[:3]
    none = [None, None, None]
    default = run_group(B, members, none, three_opts, prioritized=False)
    got = run_group(B, members, none, three_opts, prioritized=True)
    for i, (g, w) in enumerate(zip(got, default)):
        assert_psame(g, w, f"member {i}")
    # refusals of a group that is switched on
    ok = members[:2]
    pers = [PER[0], PER[2]]
    want = run_twins(B, ok, pers, lambda step, push, rc: (step(False), step(True)))
    g = B.DqnGroup.build([c for c, _ in ok], prioritized=True)
    rings = [PRing(B, c, seed, per) for (c, seed), per in zip(ok, pers)]
    bufs = [r.rb for r in rings]
    g.opt(bufs)
    store = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4, frame_stack=1), (4,), np.float32)
    empty = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4, per_config=B.PerConfig()), (4,), np.float32)
    cols = [draw(np.random.default_rng(5 + i), 4, 2, 1) for i in range(2)]
    for wrong, word in ((store, "single-frame"), (empty, "empty"), (bufs[0], "share")):
        with pytest.raises(B.BdrError) as e:
            g.opt([bufs[0], wrong])
        assert word in str(e.value), str(e.value)
        if wrong is not bufs[0]: assert "member 1" in str(e.value), str(e.value)
    for wrong, word in ((store, "single-frame"), (bufs[0], "share")):
        with pytest.raises(B.BdrError) as e:
            group_push(g, cols, 0, [bufs[0], wrong])
        assert word in str(e.value), str(e.value)
    assert _lib.lib().bdr_agent_group_set_prioritized(g.handle, 2) == 1   # BDR_ERR_INVALID
    assert g.prioritized
    # switched off: refused as by a default group, nothing advanced
    g.set_prioritized(False)
    with pytest.raises(B.BdrError) as e:
        g.opt(bufs)
    assert "member 0" in str(e.value) and "prioritized" in str(e.value)
    with pytest.raises(B.BdrError) as e:
        group_push(g, cols, 0, bufs)
    assert "member 0" in str(e.value) and "prioritized" in str(e.value)
    g.set_prioritized(True)
    losses = [rec["loss"] for rec in g.opt_with_record(bufs)]
    for i, (m, ring) in enumerate(zip(g.members, rings)):
        assert_psame(pstate(m, ring, [losses[i]]), want[i], f"member {i}")   # trees, index streams and adam_step were untouched
    assert empty.len() == 0 and store.len() == 0
    g.close()
    store.close(); empty.close()
    for ring in rings: ring.rb.close()


def test_a_nan_reward_in_one_members_ring(B, monkeypatch):
    """member 1's ring holds NaN rewards: its TD errors are NaN, the tree update is dropped and the group reports the twin's deferred
    error under the member's number; members 0 and 2 equal their twins"""
    clean_env(monkeypatch)
    members = hetero(B, 1)[:3]
    pers = [PER[0], PER[1], PER[2]]
    def poison(ring):
        n = 10
        ring.rb.push(ring.rng.standard_normal((n, ring.in_dim)).astype(np.float32), ring.rng.integers(0, ring.A, (n, 1)).astype(np.int64),
                     ring.rng.standard_normal((n, ring.in_dim)).astype(np.float32), np.full(n, np.nan, np.float32), np.zeros(n, np.int8), np.zeros(n, np.int8))
    want, messages = [], []
    for i, ((c, seed), per) in enumerate(zip(members, pers)):
        a, ring = B.Dqn.build(c), PRing(B, c, seed, per)
        if i == 1: poison(ring)
        a.opt(ring.rb); a.opt(ring.rb)
        try:
            a.sync(); messages.append(None)
        except B.BdrError as e:
            messages.append(str(e))
        want.append(pstate(a, ring, []))
        a.close(); ring.rb.close()
    assert messages[0] is None and messages[2] is None and messages[1] is not None
    g = B.DqnGroup.build([c for c, _ in members], prioritized=True)
    rings = [PRing(B, c, seed, per) for (c, seed), per in zip(members, pers)]
    poison(rings[1])
    bufs = [r.rb for r in rings]
    g.opt(bufs); g.opt(bufs)
    with pytest.raises(B.BdrError) as e:
        g.sync()
    text = messages[1].split(": ", 1)[1]          # the twin's message behind "border_amd error <code>: "
    assert "member 1: " + text in str(e.value), (str(e.value), messages[1])
    assert e.value.code == 1                      # BDR_ERR_INVALID
    g.sync()                                      # reported once
    for i, (m, r) in enumerate(zip(g.members, rings)):
        assert_psame(pstate(m, r, []), want[i], f"member {i}", finite=i != 1)
    g.close()
    for r in rings: r.rb.close()
