"""Views of a replay ring (bdr_replay_view_create, SimpleReplayBuffer.view): P index streams over ONE copy of the rows.  A view's
batch / sample_indices and a BC group's opt on views are bit for bit those of separate rings built with the same seeds and holding the
same rows; while a view lives the owner's rows are frozen."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS, CAPACITY = 300, 512


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def rows(od, ad, seed, n=N_ROWS):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32),
            rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.2).astype(np.int8), (rng.random(n) < 0.1).astype(np.int8))


def ring(B, od, ad, seed, data, per=False, capacity=CAPACITY):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed, per_config=B.PerConfig() if per else None),
                              (od,), np.float32, (ad,), np.float32, device=0)
    if data is not None:
        rb.push(*data)
    return rb


def same_batch(a, b, tag):
    for x, y, name in zip(a.unpack()[:7], b.unpack()[:7], ("obs", "act", "next_obs", "reward", "is_terminated", "is_truncated", "ix_sample")):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (tag, name)


@pytest.mark.parametrize("od", [5, 7])   # rows of 20 bytes, and of 28: neither a multiple of 16 bytes - the 4-byte gather
def test_views_sample_what_separate_rings_of_their_seeds_sample(B, od):
    data = rows(od, 3, 11)
    owner = ring(B, od, 3, 99, data)
    seeds = (1, 2, 2)
    views = [owner.view(s) for s in seeds]
    rings = [ring(B, od, 3, s, data) for s in seeds]
    assert all(len(v) == N_ROWS for v in views)
    for k in range(4):
        got = [v.batch(16) for v in views]
        want = [r.batch(16) for r in rings]
        for i in range(3):
            same_batch(got[i], want[i], (k, i))
            assert got[i].ix_sample.max() < N_ROWS
        same_batch(got[1], got[2], (k, "the two seed-2 views"))
        for v, r in zip(views, rings):
            assert np.array_equal(v.sample_indices(16), r.sample_indices(16))
    for x in views + rings: x.close()
    owner.close()


def test_a_ring_with_views_is_frozen_and_thaws_when_they_close(B):
    data, more = rows(5, 3, 11), rows(5, 3, 12, 10)
    owner, twin = ring(B, 5, 3, 99, data), ring(B, 5, 3, 99, data)
    v1, v2 = owner.view(1), owner.view(2)
    with pytest.raises(B.BdrError, match="view"):
        v1.push(*more)
    with pytest.raises(B.BdrError, match="view"):
        v1.fill_synthetic(4)
    with pytest.raises(B.BdrError, match="2 live view"):
        owner.push(*more)
    with pytest.raises(B.BdrError, match="2 live view"):
        owner.fill_synthetic(4)
    with pytest.raises(B.BdrError, match="2 live view"):
        owner.close()
    with pytest.raises(B.BdrError, match="view of a view"):
        v1.view(3)
    v1.close()
    with pytest.raises(B.BdrError, match="1 live view"):
        owner.push(*more)
    v2.close()
    owner.push(*more); twin.push(*more)
    assert len(owner) == N_ROWS + 10
    same_batch(owner.batch(16), twin.batch(16), "after the views closed")
    owner.close(); twin.close()


def test_owners_a_view_does_not_cover_are_refused(B):
    data = rows(5, 3, 11)
    per = ring(B, 5, 3, 4, data, per=True)
    with pytest.raises(B.BdrError, match="prioritized"):
        per.view(1)
    empty = ring(B, 5, 3, 4, None)
    with pytest.raises(B.BdrError, match="empty"):
        empty.view(1)
    per.push(*rows(5, 3, 12, 4))   # a refused view leaves nothing behind: the ring still takes pushes and closes
    per.close(); empty.close()


def test_a_bc_group_over_views_of_one_ring_equals_its_twins_on_three_rings(B):
    od, ad, units, bsz = 17, 6, (64, 48), 7

    def config(i):
        lr = 1e-3 * (1 + 0.5 * i)
        opt = B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
        return B.BcConfig(obs_dim=od, act_dim=ad, policy_model_config=B.BcModelConfig(B.CandleMlpConfig(units, "None"), opt), batch_size=bsz,
                          action_type="Continuous", device=0, seed=3 + i, kernel_form="general")

    def state(a, rb):
        return [a.get_params(role=r) for r in ("param", "grad", "exp_avg", "exp_avg_sq")] + [a.probe("pred", bsz), rb.sample_indices(8)]

    data = rows(od, ad, 21)
    owner = ring(B, od, ad, 99, data)
    views = [owner.view(50 + i) for i in range(3)]
    g = B.BcGroup.build([config(i) for i in range(3)])
    g.opt(views)
    recs = g.opt_with_record()
    g.opt()
    g.sync()
    for i in range(3):
        a, rb = B.Bc.build(config(i)), ring(B, od, ad, 50 + i, data)
        a.opt(rb)
        rec = a.opt_with_record(rb)
        a.opt(rb)
        a.sync()
        for x, y in zip(state(g.members[i], views[i]), state(a, rb)):
            assert np.array_equal(x, y), i
        assert np.float32(recs[i]["loss"]) == np.float32(rec["loss"])
        a.close(); rb.close()
    g.close()
    for v in views: v.close()
    owner.close()
