"""bdr_agent_group_push (DqnGroup.push): one transition per member in ONE launch, against the TWINS of tests/test_gpu_agent_group.py -
standalone agents and rings with the same configs and seeds, fed the same rows by `rb.push` of one row at a time.  Equality is `==`
on every element: ring rows, len, head, summary, index streams, batches, arenas, losses and n_opts."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_agent_group import Ring, assert_same, cfg, clean_env, hetero, state, twelve_opts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def draw(rng, in_dim, A, n):
    """n transitions as columns (the draws of tests/test_gpu_agent_group.py Ring.push, in its order)"""
    return (rng.standard_normal((n, in_dim)).astype(np.float32), rng.integers(0, A, (n, 1)).astype(np.int64),
            rng.standard_normal((n, in_dim)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < .1).astype(np.int8), (rng.random(n) < .05).astype(np.int8))


def row(cols, k):
    return tuple(c[k:k + 1] for c in cols)


def group_push(g, cols, k, bufs=None, as_array=False):
    """transition k of every member's columns, one grouped push"""
    obs = [c[0][k] for c in cols]
    nxt = [c[2][k] for c in cols]
    if as_array: obs, nxt = np.stack(obs), np.stack(nxt)
    g.push(obs, np.array([c[1][k, 0] for c in cols]), nxt, np.array([c[3][k] for c in cols], np.float32),
           np.array([c[4][k] for c in cols], np.int8), np.array([c[5][k] for c in cols], np.int8), buffers=bufs)


def ring_state(rb):
    n = rb.len()
    s = rb.summary()
    return {"rows": rb.read_rows(0, n), "len": n, "head": rb.head, "summary": (s["num_terminated_flags"], s["num_truncated_flags"], s["sum_rewards"]),
            "ixs": rb.sample_indices(40)}


def assert_same_ring(got, want, what):
    assert got["len"] == want["len"] and got["head"] == want["head"], (what, got["len"], got["head"], want["len"], want["head"])
    for name, a, b in zip(("obs", "act", "next_obs", "reward", "is_terminated", "is_truncated"), got["rows"], want["rows"]):
        assert a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all(), (what, name)
    assert got["summary"] == want["summary"], (what, "summary")
    assert (got["ixs"] == want["ixs"]).all(), (what, "index stream")


def empty_ring(B, in_dim, capacity, seed, **kw):
    return B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed, **kw), (in_dim,), np.float32)


def test_rows_land_where_a_standalone_push_puts_them(B, monkeypatch):
    """in_dim 3, 4, 4, 6, 4 (rows of 12, 16, 16, 24, 16 bytes: 4-byte, 16-byte and mixed lanes), capacities 7, 700, 64, 33, 700:
    40 grouped pushes against 40 pushes of one row; the capacity-7 ring wraps five times, the capacity-33 ring once"""
    clean_env(monkeypatch)
    h = hetero(B, 1)
    members = [h[2], h[0], h[1], h[3], h[4]]
    caps = [7, 700, 64, 33, 700]
    dims = [c.model_config.q_config.in_dim for c, _ in members]
    assert dims == [3, 4, 4, 6, 4]
    cols = [draw(np.random.default_rng(50 + i), d, c.model_config.q_config.out_dim, 40) for i, (d, (c, _)) in enumerate(zip(dims, members))]
    want = []
    for i, d in enumerate(dims):
        rb = empty_ring(B, d, caps[i], 20 + i)
        for k in range(40): rb.push(*row(cols[i], k))
        want.append(ring_state(rb))
        rb.close()
    g = B.DqnGroup.build([c for c, _ in members])
    bufs = [empty_ring(B, d, caps[i], 20 + i) for i, d in enumerate(dims)]
    group_push(g, cols, 0, bufs)
    for k in range(1, 40): group_push(g, cols, k)
    for i, rb in enumerate(bufs):
        assert_same_ring(ring_state(rb), want[i], f"member {i}")
        assert want[i]["len"] == min(40, caps[i]) and want[i]["head"] == 40 % caps[i]
    g.close()
    for rb in bufs: rb.close()


def test_staging_slots_are_reused_safely(B, monkeypatch):
    """40 grouped pushes of distinct rows back to back - no synchronise, no opt: the staging ring is rewritten five times while
    launches are still queued; a slot overwritten early is a wrong row.  (One [n, in_dim] array for all members.)"""
    clean_env(monkeypatch)
    assert 40 >= 4 * B.DqnGroup.PUSH_STAGING_DEPTH
    h = hetero(B, 1)
    members = [h[0], h[1], h[4]]
    cols = [draw(np.random.default_rng(90 + i), 4, 2, 40) for i in range(3)]
    for i, c in enumerate(cols):   # every row names its member and its step
        c[0][:, 0] = 1000 * i + np.arange(40); c[2][:, 0] = -(1000 * i + np.arange(40))
    want = []
    for i in range(3):
        rb = empty_ring(B, 4, 700, 30 + i)
        for k in range(40): rb.push(*row(cols[i], k))
        want.append(ring_state(rb))
        rb.close()
    g = B.DqnGroup.build([c for c, _ in members])
    bufs = [empty_ring(B, 4, 700, 30 + i) for i in range(3)]
    for k in range(40): group_push(g, cols, k, bufs if k == 0 else None, as_array=True)
    for i, rb in enumerate(bufs):
        got = ring_state(rb)
        assert (got["rows"][0][:, 0] == 1000 * i + np.arange(40)).all(), f"member {i}"
        assert_same_ring(got, want[i], f"member {i}")
    g.close()
    for rb in bufs: rb.close()


def test_push_and_opt_alternating_without_a_synchronise(B, monkeypatch):
    """40 iterations of (one grouped push of one row, one group opt) with no synchronise and no acting call in between: pushes and steps
    draw their launch numbers from one counter in turn, so each staging ring is rewritten five times by its own use count while the
    launches of BOTH are still queued; a slot rewritten early is a wrong row or a wrong Adam step"""
    clean_env(monkeypatch)
    assert 40 >= 4 * max(B.DqnGroup.STAGING_DEPTH, B.DqnGroup.PUSH_STAGING_DEPTH)
    members = hetero(B, 1)[:3]
    want = []
    for c, seed in members:
        a, ring = B.Dqn.build(c), Ring(B, c, seed)
        cols = draw(ring.rng, ring.in_dim, ring.A, 40)
        for k in range(40):
            ring.rb.push(*row(cols, k))
            a.opt(ring.rb)
        want.append((state(a, ring, []), ring_state(ring.rb)))
        a.close(); ring.rb.close()
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [Ring(B, c, seed) for c, seed in members]
    bufs = [r.rb for r in rings]
    cols = [draw(r.rng, r.in_dim, r.A, 40) for r in rings]
    for k in range(40):
        group_push(g, cols, k, bufs)
        g.opt(bufs)
    g.sync()
    for i, (m, r) in enumerate(zip(g.members, rings)):
        assert_same(state(m, r, []), want[i][0], f"member {i}")
        assert_same_ring(ring_state(r.rb), want[i][1], f"member {i}")
        assert m.n_opts == 40 and r.rb.len() == 340
    g.close()
    for r in rings: r.rb.close()


def test_ordering_against_the_groups_own_reads(B, monkeypatch):
    """the schedule of twelve_opts with its 50 rows pushed one by one: g.push between g.opt / g.opt_with_record against twins
    stepped by opt and fed by rb.push"""
    clean_env(monkeypatch)
    members = hetero(B, 1)
    # twins, one at a time
    want = []
    for i, (c, seed) in enumerate(members):
        a, ring = B.Dqn.build(c), Ring(B, c, seed)
        losses = []
        def step(record):
            if record: losses.append(a.opt_with_record(ring.rb)["loss"])
            else: a.opt(ring.rb)
        def push(n):
            cols = draw(ring.rng, ring.in_dim, ring.A, n)
            for k in range(n): ring.rb.push(*row(cols, k))
        twelve_opts(step, push)
        want.append(state(a, ring, losses))
        a.close(); ring.rb.close()
    # group
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [Ring(B, c, seed) for c, seed in members]
    bufs = [r.rb for r in rings]
    losses = [[] for _ in members]
    def step(record):
        if record:
            for l, rec in zip(losses, g.opt_with_record(bufs)): l.append(rec["loss"])
        else: g.opt(bufs)
    def push(n):
        cols = [draw(r.rng, r.in_dim, r.A, n) for r in rings]
        for k in range(n): group_push(g, cols, k, bufs)
    twelve_opts(step, push)
    g.sync()
    for i, (m, r) in enumerate(zip(g.members, rings)):
        assert_same(state(m, r, losses[i]), want[i], f"member {i}")
        assert len(losses[i]) == 3
    g.close()
    for r in rings: r.rb.close()


def test_ordering_against_other_streams(B, monkeypatch):
    """g.push mixed with a plain rb.push of 3 rows into member 1's ring (write after write on the ring's own stream), rb.batch(16)
    on member 2's ring (a read on the ring's own stream), member 3's own opt and group opts - against twins doing the same"""
    clean_env(monkeypatch)
    members = hetero(B, 1)
    P = len(members)
    twins = [B.Dqn.build(c) for c, _ in members]
    t_rings = [Ring(B, c, seed) for c, seed in members]
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [Ring(B, c, seed) for c, seed in members]
    bufs = [r.rb for r in rings]
    extra = np.random.default_rng(77)
    n_batches = 0
    for it in range(30):
        cols = [draw(r.rng, r.in_dim, r.A, 1) for r in rings]
        for r in t_rings: draw(r.rng, r.in_dim, r.A, 1)   # (the twins' generators stay in step)
        group_push(g, cols, 0, bufs)
        for i in range(P): t_rings[i].rb.push(*row(cols[i], 0))
        if it % 3 == 1:
            three = draw(extra, rings[1].in_dim, rings[1].A, 3)
            bufs[1].push(*three); t_rings[1].rb.push(*three)
        if it % 4 == 2:
            got, want = bufs[2].batch(16), t_rings[2].rb.batch(16)
            for a, b in zip(got.unpack()[:7], want.unpack()[:7]):
                assert (a.view(np.uint8) == b.view(np.uint8)).all(), (it, "batch")
            n_batches += 1
        if it % 5 == 3:
            g.members[3].opt(bufs[3]); twins[3].opt(t_rings[3].rb)
        if it % 6 == 4:
            g.opt(bufs)
            for a, r in zip(twins, t_rings): a.opt(r.rb)
    assert n_batches >= 5
    g.sync()
    for i in range(P):
        assert_same_ring(ring_state(bufs[i]), ring_state(t_rings[i].rb), f"member {i}")
        assert_same(state(g.members[i], rings[i], []), state(twins[i], t_rings[i], []), f"member {i}")
    g.close()
    for a in twins: a.close()
    for r in rings + t_rings: r.rb.close()


def test_more_members_than_compute_units(B, monkeypatch):
    """300 members of the CartPole shape (75 workgroups of four waves): 10 grouped pushes and one opt"""
    clean_env(monkeypatch)
    P = 300
    members = [(cfg(B, 4, (64, 64), 2, 32, param_seed=100 + i), 200 + i) for i in range(P)]
    mk = lambda c, s: Ring(B, c, s, capacity=64, first=60)   # (the pushes wrap the ring)
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [mk(c, s) for c, s in members]
    bufs = [r.rb for r in rings]
    cols = [draw(r.rng, 4, 2, 10) for r in rings]
    for k in range(10): group_push(g, cols, k, bufs if k == 0 else None, as_array=True)
    g.opt(bufs)
    g.sync()
    got = [(state(m, r, []), ring_state(r.rb)) for m, r in zip(g.members, rings)]
    g.close()
    for r in rings: r.rb.close()
    for i, (c, s) in enumerate(members):
        a, ring = B.Dqn.build(c), mk(c, s)
        tc = draw(ring.rng, 4, 2, 10)
        assert all((x == y).all() for x, y in zip(tc, cols[i]))
        for k in range(10): ring.rb.push(*row(tc, k))
        a.opt(ring.rb)
        want = (state(a, ring, []), ring_state(ring.rb))
        a.close(); ring.rb.close()
        assert_same(got[i][0], want[0], f"member {i}")
        assert_same_ring(got[i][1], want[1], f"member {i}")


def test_refusals_leave_nothing_behind(B, monkeypatch):
    """every refusal with a valid member 0: no ring's len, head or index stream moves"""
    clean_env(monkeypatch)
    from border_amd import _lib
    ok = hetero(B, 1)[:2]
    g = B.DqnGroup.build([c for c, _ in ok])
    rings = [Ring(B, c, seed, first=30) for c, seed in ok]
    twins = [Ring(B, c, seed, first=30) for c, seed in ok]
    bufs = [r.rb for r in rings]
    cols = [draw(np.random.default_rng(5 + i), 4, 2, 2) for i in range(2)]
    group_push(g, cols, 0, bufs)
    for i in range(2): twins[i].rb.push(*row(cols[i], 0))
    per = empty_ring(B, 4, 700, 4, per_config=B.PerConfig())
    store = empty_ring(B, 4, 700, 4, frame_stack=1)
    wide = empty_ring(B, 6, 700, 4)
    two_acts = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4), (4,), np.float32, act_shape=(2,))
    wrong = [(per, "prioritized"), (store, "single-frame"), (wide, "do not match"), (two_acts, "i64"), (bufs[0], "share")]
    other = None
    if B.device_count() > 1:
        other = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4), (4,), np.float32, device=1)
        wrong.append((other, "another device"))
    for rb, word in wrong:
        with pytest.raises(B.BdrError) as e:
            group_push(g, cols, 1, [bufs[0], rb])
        assert word in str(e.value), str(e.value)
        if rb is not bufs[0]: assert "member 1" in str(e.value), str(e.value)
    # null pointers: through the C entry itself
    vp = C.c_void_p
    o = [np.ascontiguousarray(c[0][1]) for c in cols]; x = [np.ascontiguousarray(c[2][1]) for c in cols]
    act, rew, flag = np.zeros(2, np.int64), np.zeros(2, np.float32), np.zeros(2, np.int8)
    good_b, good_o, good_x = (vp * 2)(*[b.handle for b in bufs]), (vp * 2)(*[a.ctypes.data for a in o]), (vp * 2)(*[a.ctypes.data for a in x])
    p = lambda a: a.ctypes.data_as(vp)
    for b_, o_, x_ in (((vp * 2)(bufs[0].handle, None), good_o, good_x), (good_b, (vp * 2)(o[0].ctypes.data, None), good_x),
                       (good_b, good_o, (vp * 2)(x[0].ctypes.data, None)), (None, good_o, good_x)):
        assert _lib.lib().bdr_agent_group_push(g.handle, b_, o_, p(act), x_, p(rew), p(flag), p(flag)) != 0
    for i in range(2):
        assert bufs[i].len() == twins[i].rb.len() == 31 and bufs[i].head == twins[i].rb.head, i
    for rb in (per, store, wide, two_acts): assert rb.len() == 0 and rb.head == 0
    # and the accepted call after them lands where it would have
    group_push(g, cols, 1, bufs)
    for i in range(2): twins[i].rb.push(*row(cols[i], 1))
    for i in range(2):
        assert_same_ring(ring_state(bufs[i]), ring_state(twins[i].rb), f"member {i}")
    g.close()
    for rb in [per, store, wide, two_acts] + ([other] if other else []): rb.close()
    for r in rings + twins: r.rb.close()
