"""The "online" scenario of tests/test_gpu_candle_sac_group.py, and its AWAC counterpart, with the rows going in through the GROUPED
push: after every round every member's ring takes 7 new rows through CandleSacGroup.push / AwacGroup.push (one launch for all members),
the twins' rings through rb.push.  Shapes `partial_block` and `one_action`, P = 3, 11 rounds, round 5 an opt_with_record; member 1 takes
an update_on_batch of its own after round 6.  After the last round the members' state (arenas by role, probes, step counters, the noise
counter via the trailing draws, the index stream), the records and the rings equal the twins' bit for bit.  The rings (capacity 128,
100 rows) are full after round 4 and wrap from then on.
`own_push`: member 1 also pushes 3 rows through its own rb.push - on the ring's own stream - after every odd round, between the grouped
pushes: the ring's event orders the two streams."""
import functools

import numpy as np
import pytest

from tests import test_gpu_awac_group as TA
from tests import test_gpu_candle_sac_group as TC
from tests.test_gpu_group_push import assert_same_ring, ring_state

pytestmark = pytest.mark.gpu

ROUNDS, RECORD_ROUND, OWN_UPDATE_AFTER, PUSH_ROWS, P = 11, 5, 6, 7, 3
KINDS = {
    "awac": (TA, "Awac", "AwacGroup", {"partial_block": TA.SHAPES["partial_block"],
                                       "one_action": (3, 1, (64, 64), (64, 64), "None", 2, 34, ("Tanh", "Mse", False))}),
    "candle_sac": (TC, "CandleSac", "CandleSacGroup", {n: TC.SHAPES[n] for n in ("partial_block", "one_action")}),
}


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def pushed_rows(mod, shape, i, k, n=PUSH_ROWS):
    """the rows member i's ring takes after round k"""
    return mod.rows(shape, 9000 + 100 * i + k, n)


def own_rows(mod, shape, k):
    return mod.rows(shape, 12000 + k, 3)


@functools.lru_cache(maxsize=None)
def twin(kind, name, i, own, own_push):
    """member i's twin, stepped alone and fed by rb.push: (state, the record of round 5, its ring)"""
    import border_amd as B
    mod, agent, _, shapes = KINDS[kind]
    shape = shapes[name]
    a, rb = getattr(B, agent).build(mod.config(B, shape, i)), mod.ring(B, shape, 100 + i)
    rec = None
    for k in range(1, ROUNDS + 1):
        if k == RECORD_ROUND: rec = a.opt_with_record(rb)
        else: a.opt(rb)
        if k == OWN_UPDATE_AFTER and own: a.update_on_batch(*mod.own_batch(shape, i))
        rb.push(*pushed_rows(mod, shape, i, k))
        if own_push and own and k % 2 == 1: rb.push(*own_rows(mod, shape, k))
    a.sync()
    out = (mod.state(a, rb, shape), rec, ring_state(rb))
    a.close(); rb.close()
    return out


def run_group(B, kind, name, own_push=False):
    mod, _, group, shapes = KINDS[kind]
    shape = shapes[name]
    own = 1
    g = getattr(B, group).build([mod.config(B, shape, i) for i in range(P)])
    rings = [mod.ring(B, shape, 100 + i) for i in range(P)]
    count = mod.launch_count(shape)
    recs = None
    for k in range(1, ROUNDS + 1):
        if k == RECORD_ROUND: recs = g.opt_with_record()
        else: g.opt(rings if k == 1 else None)
        if k == OWN_UPDATE_AFTER: g.members[own].update_on_batch(*mod.own_batch(shape, own))
        cols = [pushed_rows(mod, shape, i, k) for i in range(P)]
        g.push(*[[c[f] for c in cols] for f in (0, 1, 2, 3, 4, 5)])
        if own_push and k % 2 == 1: rings[own].push(*own_rows(mod, shape, k))
    g.sync()
    assert g.kernel_launches == ROUNDS * (count + 1)   # rounds x count, and one launch per grouped push
    for i, (m, rb) in enumerate(zip(g.members, rings)):
        want, want_rec, want_ring = twin(kind, name, i, i == own, own_push)
        got, got_ring = mod.state(m, rb, shape), ring_state(rb)   # (the twin's order: both draw from the ring's index stream)
        assert_same_ring(got_ring, want_ring, (kind, name, i))
        mod.assert_same(got, want, (kind, name, i))
        assert list(recs[i]) == list(mod.KEYS) and mod.rec_bits(recs[i]) == mod.rec_bits(want_rec), (kind, name, i, recs[i], want_rec)
        assert m.n_opts == ROUNDS + (1 if i == own else 0)
    g.close()
    for rb in rings: rb.close()


@pytest.mark.parametrize("name", ["one_action", "partial_block"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rounds_after_grouped_pushes_see_the_new_size_and_rows(B, kind, name):
    assert TC.N_ROWS + 4 * PUSH_ROWS == 128 and TC.N_ROWS + ROUNDS * PUSH_ROWS > 128   # full after round 4, wrapped by the end
    run_group(B, kind, name)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_members_own_push_on_the_rings_stream_between_grouped_pushes(B, kind):
    run_group(B, kind, "partial_block", own_push=True)
