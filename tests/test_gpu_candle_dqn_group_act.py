"""CandleDqnGroup.sample (bdr_candle_dqn_group_sample / _sample_members: ONE launch of k_cdqn_act_group, then every selected member's
own explorer on the host) against twins: standalone CandleDqn agents with the same configs, called one after the other through
sample_raw on the layer path and on the fused path.  Everything is == on the raw values.

Three members, one per explorer rule: member 0 Softmax in train mode (reads the Q rows), member 1 epsilon-greedy in train mode with
record_verbose_level 2 (reads the indices; n_samples_best_act counts), member 2 in eval mode (the 1-in-100 random action, else the
index).  The Q rows a call brought back (last_q) are compared with the twins' own action values in every combination of n, dtype and
normaliser, so the float64 conversion and the normaliser in front of the first layer have a bit check on the values, not only on
the action picked.  The Softmax rule runs the library's one host softmax on the Q rows the device returned, on both sides: no host expf difference
can enter.  Shapes: (obs 4, A 2, [64, 64]) and (obs 70, A 33, [128]) - an odd number of actions, so that the members' result blocks
([n] i64 indices, then [n][A] floats, rows padded to an even number of floats) need their padding to stay 8-byte aligned.
n = 1, 8, 9 and 33 rows: one row, a partial block, two blocks with one row in the second."""
import numpy as np
import pytest

from tests.test_gpu_candle_dqn_group import SHAPES, bits, config, ring

pytestmark = pytest.mark.gpu

ACT_SHAPES = ("cartpole_small", "odd_double")
P = 3


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def act_config(B, shape, i):
    ex = B.EpsilonGreedy(eps_start=0.9, eps_final=0.1, final_step=50) if i == 1 else B.Softmax()
    return config(B, shape, i, train=(i != 2), explorer=ex, record_verbose_level=2 if i == 1 else 0)


def build(B, name, path):
    shape = SHAPES[name]
    g = B.CandleDqnGroup.build([act_config(B, shape, i) for i in range(P)])
    twins = [B.CandleDqn.build(act_config(B, shape, i)) for i in range(P)]
    for t in twins: t.set_act_path(path)
    return g, twins


def obs_rows(shape, n, seed, dtype=np.float32):
    return (0.5 + np.random.default_rng(seed).standard_normal((n, shape[0]))).astype(dtype)


def bookkeeping(a, obs):
    """the member's counters after one more call of its own (which also shows where its explorer stream stands)"""
    act, info = a.sample(obs, return_info=True)
    return act.tolist(), info["eps"], info["is_random"], info["n_samples_act"], info["n_samples_best_act"], a.explorer_state()["n_opts"]


@pytest.mark.parametrize("path", ["layers", "fused"])
@pytest.mark.parametrize("name", ACT_SHAPES)
def test_actions_and_q_rows_equal_every_members_own_call(B, name, path):
    shape = SHAPES[name]
    O, A = shape[0], shape[1]
    g, twins = build(B, name, path)
    k = np.arange(O)
    norm = B.ObsNormalizer(O, 0).set((0.5 + 0.01 * k).astype(np.float32), (1.0 + 0.125 * (k % 4)).astype(np.float32))
    call = 0
    for n in (1, 8, 9, 33):
        for dtype in (np.float32, np.float64):
            for nm in (None, norm):
                call += 1
                rows = [obs_rows(shape, n, 100 * call + i, dtype) for i in range(P)]
                launches = g.kernel_launches
                got = g.sample(rows, norm=nm)
                assert g.kernel_launches == launches + 1                          # one launch per call
                for i in range(P):
                    want = twins[i].sample_raw(rows[i], nm)
                    assert got[i].dtype == np.int64 and got[i].shape == (n,) and (got[i] == want).all(), (n, dtype, nm is not None, i)
                    assert ((0 <= got[i]) & (got[i] < A)).all()
                    # the Q rows the explorer read, in every combination: the twin's own action values on the f32 form of the rows -
                    # float64 rows rounded to f32, normalised rows as ObsNormalizer.apply gives them, the bits the twin's own
                    # sample_raw puts in front of its first layer (tests/test_gpu_candle_dqn.py holds the two equal)
                    f32 = rows[i].astype(np.float32)
                    want_q = twins[i].qvalues(f32 if nm is None else nm.apply(f32))
                    got_q = g.last_q(i, n)
                    assert got_q.shape == (n, A) and (bits(got_q) == bits(want_q)).all(), (n, dtype, nm is not None, i)
    obs = obs_rows(shape, 4, 7)
    for i in range(P):
        assert bookkeeping(g.members[i], obs) == bookkeeping(twins[i], obs), i
    g.close(); norm.close()
    for t in twins: t.close()


@pytest.mark.parametrize("name", ACT_SHAPES)
def test_one_explorer_stream_across_group_calls_subset_calls_own_calls_and_rounds(B, name):
    shape = SHAPES[name]
    g, twins = build(B, name, "fused")
    bufs, tbufs = [ring(B, shape, 100 + i) for i in range(P)], [ring(B, shape, 100 + i) for i in range(P)]
    step = 0

    def rows(n):
        nonlocal step
        step += 1
        return [obs_rows(shape, n, 1000 * step + i) for i in range(P)]

    def group_call(n, members=None):
        r = rows(n)
        launches = g.kernel_launches
        got = g.sample(r, members=members)
        assert g.kernel_launches == launches + 1                                  # one launch whatever the selection
        for i in range(P):
            if members is not None and i not in members:
                assert got[i] is None                                              # not selected: it acts not, and draws nothing (below)
                continue
            assert (got[i] == twins[i].sample_raw(r[i])).all(), (step, i)

    def own_call(i, n):
        r = rows(n)
        assert (g.members[i].sample_raw(r[i]) == twins[i].sample_raw(r[i])).all(), (step, i)

    def round_():
        g.opt(bufs)
        for i in range(P): twins[i].opt(tbufs[i])

    for _ in range(3):
        group_call(2)
        group_call(3, members=[0, 2])
        own_call(1, 2)
        round_()
        group_call(1, members=[1])
        own_call(0, 5)
        group_call(9)
        group_call(1, members=[2])
    g.sync()
    for t in twins: t.sync()
    obs = obs_rows(shape, 4, 7)
    for i in range(P):
        assert bookkeeping(g.members[i], obs) == bookkeeping(twins[i], obs), i     # the stream, the epsilon counter, both sample counters
        for k in ("qnet", "qnet_tgt"):
            assert (bits(g.members[i].get_params(k)) == bits(twins[i].get_params(k))).all(), (i, k)
    # ratio_best_act of the next record is the twins': the counters a group call moved are the ones opt_with_record reads and resets
    recs = g.opt_with_record(bufs)
    for i in range(P):
        want = twins[i].opt_with_record(tbufs[i])
        assert [(k, np.float32(v).view(np.uint32)) for k, v in recs[i].items()] == [(k, np.float32(v).view(np.uint32)) for k, v in want.items()], i
    for i in range(P):
        assert bookkeeping(g.members[i], obs) == bookkeeping(twins[i], obs), i
    g.close()
    for x in twins + bufs + tbufs: x.close()


def test_refused_acting_calls_move_nothing(B):
    shape = SHAPES["cartpole_small"]
    g, twins = build(B, "cartpole_small", "fused")
    r = [obs_rows(shape, 2, 5 + i) for i in range(P)]
    launches = g.kernel_launches
    with pytest.raises(B.BdrError, match="strictly ascending"):
        g.sample(r, members=[2, 0])
    with pytest.raises(B.BdrError, match="member 3"):
        g.sample(r, members=[0, 3])
    with pytest.raises(B.BdrError, match="member 1: null observation rows"):
        g.sample([r[0], None, r[2]])
    assert g.kernel_launches == launches
    obs = obs_rows(shape, 4, 7)
    for i in range(P):
        assert bookkeeping(g.members[i], obs) == bookkeeping(twins[i], obs), i
    g.close()
    for t in twins: t.close()
