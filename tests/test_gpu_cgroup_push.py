"""bdr_awac_group_push / bdr_candle_sac_group_push (AwacGroup.push, CandleSacGroup.push): n transitions per member in ONE launch,
against TWINS - rings with the same configs and seeds, fed the same rows as float32 through `rb.push`.  Equality is `==` on bytes:
ring rows, len, head, summary and the index stream (ring_state / assert_same_ring of tests/test_gpu_group_push.py), after EVERY push.

Rings have capacity 16.  Shapes (obs, act), the smallest at which the copy lanes differ:
  (3, 1)     rows of 12 and 4 bytes: 4-byte lanes only
  (17, 6)    rows of 68 and 24 bytes: 16-byte lanes plus a 4-byte tail
  (45, 24)   the pen record
Group sizes 1 and 5 (four waves share a workgroup: 5 reaches a partial last one).  Even members push float32 rows, odd members float64
rows (converted on the device; the twin takes astype(np.float32)).  The sequence: 30 single-row pushes - the ring wraps after 16, the
push staging ring of 8 slots is rewritten three times, and the head ends at 14 -, then one push of n = 3 that crosses the wrap (rows
14, 15, 0), then one push of push_max_rows() rows - the slot bound, several times the ring's capacity - and one row more is refused.
kernel_launches moves by exactly one per push."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_awac_group as TA
from tests import test_gpu_candle_sac_group as TC
from tests.test_gpu_group_push import assert_same_ring, ring_state

pytestmark = pytest.mark.gpu

CAPACITY, SINGLES = 16, 30
KINDS = {
    "awac": (TA, "AwacGroup", lambda od, ad: (od, ad, (64, 48), (64, 48), "None", 2, 7, ("Clamp", "Mse", False))),
    "candle_sac": (TC, "CandleSacGroup", lambda od, ad: (od, ad, (64, 48), (64, 48), "None", 2, 7, ("Clamp", "Mse"), "Mlp2", 1.0)),
}
DIMS = [(3, 1), (17, 6), (45, 24)]


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def build(B, kind, od, ad, P):
    mod, cls, shape = KINDS[kind]
    return getattr(B, cls).build([mod.config(B, shape(od, ad), i) for i in range(P)])


def empty_ring(B, od, ad, seed, capacity=CAPACITY, **kw):
    return B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed, **kw), (od,), np.float32, (ad,), np.float32, device=0)


def draw(rng, od, ad, n, dtype):
    """n transitions as columns; observation rows in `dtype` (float64 rows carry bits float32 cannot hold)"""
    return (rng.standard_normal((n, od)).astype(dtype), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32), rng.standard_normal((n, od)).astype(dtype),
            rng.standard_normal(n).astype(np.float32), (rng.random(n) < .2).astype(np.int8), (rng.random(n) < .1).astype(np.int8))


def as_f32(cols):
    return (cols[0].astype(np.float32), cols[1], cols[2].astype(np.float32)) + tuple(cols[3:])


def group_push(g, cols, bufs=None):
    """cols[i]: member i's columns (obs, act, next_obs, reward, is_terminated, is_truncated)"""
    g.push([c[0] for c in cols], [c[1] for c in cols], [c[2] for c in cols], [c[3] for c in cols], [c[4] for c in cols], [c[5] for c in cols], buffers=bufs)


def dtype_of(i):
    return np.float32 if i % 2 == 0 else np.float64


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_push_leaves_the_rings_as_a_standalone_push_does(B, kind, dims, P):
    od, ad = dims
    g = build(B, kind, od, ad, P)
    bufs = [empty_ring(B, od, ad, 20 + i) for i in range(P)]
    twins = [empty_ring(B, od, ad, 20 + i) for i in range(P)]
    rngs = [np.random.default_rng(50 + i) for i in range(P)]
    launches = g.kernel_launches

    def push(n, what):
        nonlocal launches
        cols = [draw(rngs[i], od, ad, n, dtype_of(i)) for i in range(P)]
        group_push(g, cols, bufs)
        for i in range(P): twins[i].push(*as_f32(cols[i]))
        launches += 1
        assert g.kernel_launches == launches, what
        for i in range(P): assert_same_ring(ring_state(bufs[i]), ring_state(twins[i]), (what, f"member {i}"))

    assert SINGLES >= 21 and SINGLES > 3 * g.PUSH_STAGING_DEPTH and SINGLES % CAPACITY == CAPACITY - 2
    for k in range(SINGLES): push(1, f"single push {k}")
    assert bufs[0].head == CAPACITY - 2 and bufs[0].len() == CAPACITY
    push(3, "n = 3 across the wrap")
    assert bufs[0].head == 1
    n_max = g.push_max_rows([dtype_of(i) for i in range(P)])
    assert n_max > CAPACITY
    push(n_max, f"n = {n_max}, the slot bound")
    cols = [draw(np.random.default_rng(1), od, ad, n_max + 1, dtype_of(i)) for i in range(P)]
    with pytest.raises(B.BdrError) as e:
        group_push(g, cols, bufs)
    assert "split" in str(e.value), str(e.value)
    assert g.kernel_launches == launches
    push(2, "after the refusal")
    g.close()
    for rb in bufs + twins: rb.close()


CRAFTED = np.array([0.1, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1e-40, 1e-46, 3.5e38, -0.0, np.inf, -np.inf, np.nan, -1e-40, -3.5e38, 2.0 ** -149, 2.0 ** -150,
                    1.5 * 2.0 ** -149, 3.4028235677973366e38, 1 - 2.0 ** -25], np.float64)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_float64_rows_are_rounded_once_to_nearest_even(B, kind):
    """the crafted values in every column position of obs and next_obs: bytes of astype(np.float32), NaN by isnan"""
    od, ad = 17, 6
    g = build(B, kind, od, ad, 2)
    bufs = [empty_ring(B, od, ad, 7 + i) for i in range(2)]
    n = 4
    obs = np.stack([np.roll(CRAFTED, j) for j in range(n)])
    nxt = np.stack([np.roll(-CRAFTED, j + 5) for j in range(n)])
    assert obs.shape == (n, od)
    act, rew, flag = np.zeros((n, ad), np.float32), np.arange(n, dtype=np.float32), np.zeros(n, np.int8)
    g.push(obs, act, nxt, rew, flag, flag, buffers=bufs)   # one float64 array for both members
    with np.errstate(over="ignore"):
        want_o, want_x = obs.astype(np.float32), nxt.astype(np.float32)
    assert np.isinf(want_o).sum() >= 3 * n and (want_o == 0).sum() >= 2 * n   # (the overflow and the underflow really happen)
    for rb in bufs:
        got = rb.read_rows(0, n)
        for a, b in ((got[0], want_o), (got[2], want_x)):
            nan = np.isnan(b)
            assert nan.sum() == n and (np.isnan(a) == nan).all()
            assert (a.view(np.uint32)[~nan] == b.view(np.uint32)[~nan]).all()
    g.close()
    for rb in bufs: rb.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_refusals_leave_nothing_behind(B, kind):
    """every refusal with a valid member 0: no ring's len, head, rows or index stream moves, nor does kernel_launches, and the next
    valid push lands where it would have"""
    from border_amd import _lib
    od, ad = 17, 6
    g = build(B, kind, od, ad, 2)
    bufs = [empty_ring(B, od, ad, 30 + i) for i in range(2)]
    twins = [empty_ring(B, od, ad, 30 + i) for i in range(2)]
    rng = np.random.default_rng(3)
    first = [draw(rng, od, ad, 5, np.float32) for _ in range(2)]
    group_push(g, first, bufs)
    for i in range(2): twins[i].push(*first[i])
    launches = g.kernel_launches
    cols = [draw(rng, od, ad, 2, np.float32) for _ in range(2)]
    owner = empty_ring(B, od, ad, 4)
    owner.push(*draw(rng, od, ad, 3, np.float32))
    view = owner.view(9)
    wrong = [(None, "null buffer"), (view, "view"), (owner, "live view"), (empty_ring(B, od, ad, 4, per_config=B.PerConfig()), "prioritized"),
             (empty_ring(B, 16, ad, 4, frame_stack=1), "single-frame"), (empty_ring(B, od, ad, 4, index_rng="xoshiro256++"), "StdRng"),
             (empty_ring(B, od + 1, ad, 4), "do not match"), (empty_ring(B, od, ad + 1, 4), "do not match"), (bufs[0], "shares")]
    if B.device_count() > 1:
        wrong.append((B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=CAPACITY, seed=4), (od,), np.float32, (ad,), np.float32, device=1), "another device"))
    before = [(rb, rb.len(), rb.head) for rb, _ in wrong if rb is not None and rb is not bufs[0]]
    for rb, word in wrong:
        with pytest.raises(B.BdrError) as e:
            group_push(g, cols, [bufs[0], rb])
        assert word in str(e.value) and "member 1" in str(e.value), (word, str(e.value))
    # null row pointers, n = 0 and an unknown dtype: through the C entry itself
    vp = C.c_void_p
    fn = getattr(_lib.lib(), f"bdr_{kind}_group_push")
    arrs = [[np.ascontiguousarray(c[f]) for c in cols] for f in range(6)]
    good = [(vp * 2)(*[a.ctypes.data for a in arrs[f]]) for f in range(6)]
    hb = (vp * 2)(*[b.handle for b in bufs])
    f32 = (C.c_int32 * 2)(_lib.BDR_DTYPE_F32, _lib.BDR_DTYPE_F32)

    def call(n=2, b=hb, dt=f32, **null):
        a = [(vp * 2)(arrs[f][0].ctypes.data, None) if null.get("f") == f else good[f] for f in range(6)]
        return fn(g.handle, b, n, a[0], a[2], dt, a[1], a[3], a[4], a[5])
    for f in range(6):
        assert call(f=f) != 0 and "member 1" in _lib.lib().bdr_last_error().decode()
    assert call(n=0) != 0
    assert call(dt=(C.c_int32 * 2)(_lib.BDR_DTYPE_F32, 7)) != 0 and "dtype" in _lib.lib().bdr_last_error().decode()
    assert call(b=None) != 0
    assert g.kernel_launches == launches
    for rb, n, head in before: assert rb.len() == n and rb.head == head
    for i in range(2): assert_same_ring(ring_state(bufs[i]), ring_state(twins[i]), f"member {i} after the refusals")
    assert call() == 0   # (and the accepted call, through the same path)
    for i in range(2): twins[i].push(*cols[i])
    assert g.kernel_launches == launches + 1
    for i in range(2): assert_same_ring(ring_state(bufs[i]), ring_state(twins[i]), f"member {i}")
    g.close()
    view.close()
    for rb, _ in wrong:
        if rb is not None and rb is not bufs[0] and rb is not view: rb.close()
    for rb in bufs + twins: rb.close()
