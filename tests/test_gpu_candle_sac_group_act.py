"""CandleSacGroup.sample (csrc/candle_act_group.hpp k_candle_act_group through the C ABI, with CandleActKind of a CandleSac): every
selected member gets the bits of its own bdr_agent_sample_raw in the mode it is in, at the noise counter it is at (np.array_equal on
the raw bits throughout).  SAC members are the first whose actor may be an Mlp2: the last layer is [mean | s], 2 A wide, and the
epilogue reads s at column A + j of the row.

In eval mode a member's own call moves nothing, so the group is compared against the members themselves, on the layer path and on the
one-launch path.  In train mode every call takes draws, so the group is compared against TWINS: standalone CandleSac agents built from
the same configs, which make the standalone calls of exactly the calls their member took part in.

Shapes (obs, act, actor units, actor kind; the critic is (64,), two critics): the five of tests/test_gpu_candle_sac_group.py, and
  21  65  (64, 40)   Mlp2  a last layer of 130 columns padded to 192, A not a multiple of 32
  9   4   (480, 64)  Mlp2  W = 512 > 448: the one-team entry k_candle_act_group<1>; Kp = 512 > 256: the in-tile weight loads
with P = 1, 2, 5 members and n = 1, 32, 33 rows: one block, a full block, two blocks with one row in the second.  Member i differs from
member 0 in seed, action limit (Clamp with its own bounds for even i, Tanh with its own scale for odd i) and the log-std clamps.  The
output blocks of members that are not selected keep their sentinel."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {
    "partial_block": (17, 6, (64, 48), "Mlp2"),
    "pen": (45, 24, (256, 256), "Mlp2"),
    "no_hidden": (9, 4, (64,), "Mlp3"),
    "wide_action": (21, 70, (128,), "Mlp3"),
    "one_action": (3, 1, (64, 64), "Mlp2"),
    "mlp2_wide_out": (21, 65, (64, 40), "Mlp2"),
    "mlp2_one_team": (9, 4, (480, 64), "Mlp2"),
}
NS = (1, 32, 33)
SENTINEL = np.float32(-7777.25)
BATCH = 8


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def config(B, shape, i, log_std=None):
    from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, MultiCriticConfig
    od, ad, un, kind = shape
    opt = lambda: B.OptimizerConfig.Adam(1e-3 * (1 + 0.5 * i))
    limit = ActionLimit.Tanh(1.0 + 0.25 * i) if i % 2 else ActionLimit.Clamp(-0.5 - 0.1 * i, 0.6 + 0.1 * i)
    lo, hi = log_std if log_std is not None else (-3.0 + 0.5 * i, 1.0 - 0.2 * i)
    return B.CandleSacConfig(obs_dim=od, act_dim=ad, critic_config=MultiCriticConfig(2, CandleMlpConfig((64,)), opt(), 0.005),
                             actor_config=GaussianActorConfig(CandleMlpConfig(tuple(un)), opt(), min_log_std=lo, max_log_std=hi, action_limit=limit, kind=kind),
                             ent_coef_mode=B.EntCoefMode.Auto(-float(ad), 1e-3) if i % 2 else B.EntCoefMode.Fix(0.2), batch_size=BATCH, seed=3 + i, device=0)


def group(B, shape, P, **kw):
    return B.CandleSacGroup.build([config(B, shape, i, **kw) for i in range(P)])


def twins(B, shape, P, **kw):
    return [B.CandleSac.build(config(B, shape, i, **kw)) for i in range(P)]


def normaliser(B, O, seed=0):
    rng = np.random.default_rng(900 + seed)
    return B.ObsNormalizer(O, 0).set(rng.standard_normal(O).astype(np.float32), rng.uniform(0.5, 2.0, O).astype(np.float32))


def rows_for(shape, P, n, dtype, seed=0):
    rng = np.random.default_rng(77 + seed)
    return [(3.0 * rng.standard_normal((n, shape[0]))).astype(dtype) for _ in range(P)]


def own(member, rows, norm):
    """an EVAL-mode member's own bdr_agent_sample_raw on both act paths: one result, the two paths hold the same bits"""
    assert not member.is_train()
    out = []
    for path in ("layers", "fused"):
        member.set_act_path(path)
        out.append(member.sample_raw(rows, norm))
    member.set_act_path("default")
    assert np.array_equal(out[0], out[1])
    return out[0]


def twin_call(twin, rows, norm=None, path="layers"):
    twin.set_act_path(path)
    return twin.sample_raw(rows, norm)


@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_eval_mode_group_sample_equals_each_members_own_sample_raw(B, name, P):
    shape = SHAPES[name]
    g = group(B, shape, P)
    nz = normaliser(B, shape[0])
    for n in NS:
        for dtype in (np.float32, np.float64):
            for norm in (None, nz):
                rows = rows_for(shape, P, n, dtype, seed=n)
                before = g.kernel_launches
                got = g.sample(rows, norm)
                assert g.kernel_launches == before + 1                      # ONE launch per call, whatever P and n
                for i, m in enumerate(g.members):
                    want = own(m, rows[i], norm)
                    assert got[i].shape == (n, shape[1]) and np.array_equal(got[i], want), (name, P, n, dtype, norm is not None, i)
    assert all(m.n_opts == 0 for m in g.members)
    g.close(); nz.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_train_mode_mirrored_sequence_against_twins(B, name):
    """a group call with n = 33, member 1's own sample_raw with n = 1, a group call over members [0, 2] with n = 32, a group call over all
    with n = 1: twin i makes the standalone calls of exactly the calls member i took part in, so equal bits at every step fix the advance
    of exactly n * A per selected member and the untouched counters of the others"""
    shape, P = SHAPES[name], 3
    g, tw = group(B, shape, P), twins(B, shape, P)
    for a in g.members + tw: a.train()
    nz = normaliser(B, shape[0])
    r33 = rows_for(shape, P, 33, np.float64, seed=1)
    got = g.sample(r33, nz)
    for i in range(P):
        assert np.array_equal(got[i], twin_call(tw[i], r33[i], nz, "layers")), (name, "n33", i)
    one = rows_for(shape, 1, 1, np.float32, seed=2)[0]
    for path in ("layers", "fused"):                                        # the member's own calls on either path continue the stream
        g.members[1].set_act_path(path)
        assert np.array_equal(g.members[1].sample_raw(one), twin_call(tw[1], one, None, path)), (name, "own", path)
    r32 = rows_for(shape, P, 32, np.float32, seed=3)
    got = g.sample([r32[0], None, r32[2]], members=[0, 2])
    assert got[1] is None
    for i in (0, 2):
        assert np.array_equal(got[i], twin_call(tw[i], r32[i], None, "fused")), (name, "n32", i)
    r1 = rows_for(shape, P, 1, np.float32, seed=4)
    before = g.kernel_launches
    got = g.sample(r1)
    assert g.kernel_launches == before + 1
    for i in range(P):
        assert np.array_equal(got[i], twin_call(tw[i], r1[i], None, "layers")), (name, "n1", i)
    # bdr_agent_noise continues the same stream: the next draws of member and twin are the same
    for i in range(P):
        assert np.array_equal(g.members[i].draw_noise(5), tw[i].draw_noise(5)), i
    # one call with member 0 in eval mode and members 1, 2 in train mode
    g.members[0].eval(); tw[0].eval()
    r5 = rows_for(shape, P, 33, np.float32, seed=5)
    got = g.sample(r5)
    for i in range(P):
        assert np.array_equal(got[i], twin_call(tw[i], r5[i], None, "layers")), (name, "mixed", i)
    assert np.array_equal(got[0], own(g.members[0], r5[0], None))           # eval: the mean, and no draw taken ...
    got = g.sample(r5)
    assert np.array_equal(got[0], twin_call(tw[0], r5[0]))                  # ... so eval repeats, while the members in train mode moved on
    for i in (1, 2):
        assert np.array_equal(got[i], twin_call(tw[i], r5[i])), i
    assert all(m.n_opts == 0 for m in g.members)
    g.close(); nz.close()
    for t in tw: t.close()


def raw_call(B, g, members, n, rows, codes, outs, norms=None):
    """bdr_candle_sac_group_sample_members as the C caller sees it: every array indexed by member"""
    from border_amd import _lib
    P = len(g)
    ptr = lambda a: None if a is None else a.ctypes.data
    rp, op = (C.c_void_p * P)(*[ptr(r) for r in rows]), (C.c_void_p * P)(*[ptr(o) for o in outs])
    cp = (C.c_int32 * P)(*codes)
    np_ = None if norms is None else (C.c_void_p * P)(*[None if z is None else z.handle for z in norms])
    if members is None:
        return _lib.lib().bdr_candle_sac_group_sample(g.handle, np_, n, rp, cp, op)
    sel = np.asarray(members, np.uint32)
    return _lib.lib().bdr_candle_sac_group_sample_members(g.handle, sel.ctypes.data_as(C.c_void_p), sel.size, np_, n, rp, cp, op)


def test_a_subset_selection_leaves_the_other_members_untouched(B):
    shape, P, n = SHAPES["partial_block"], 5, 33
    g = group(B, shape, P)
    rows = rows_for(shape, P, n, np.float32)
    outs = [np.full((n, shape[1]), SENTINEL, np.float32) for _ in range(P)]
    before = g.kernel_launches
    assert raw_call(B, g, [0, 3], n, rows, [0] * P, outs) == 0
    assert g.kernel_launches == before + 1
    for i, m in enumerate(g.members):
        if i in (0, 3): assert np.array_equal(outs[i], own(m, rows[i], None)), i
        else: assert np.all(outs[i] == SENTINEL), i
        assert m.n_opts == 0
    got = g.sample([rows[0], None, None, rows[3], None], members=[0, 3])
    assert [x is None for x in got] == [False, True, True, False, True] and np.array_equal(got[3], outs[3])
    all_a, all_b = g.sample(rows), g.sample(rows, members=list(range(P)))
    assert all(np.array_equal(a, b) for a, b in zip(all_a, all_b))
    g.close()


def transitions(shape, n, seed):
    od, ad = shape[0], shape[1]
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32),
            rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal(n).astype(np.float32), np.zeros(n, np.int8), np.zeros(n, np.int8))


def test_actions_follow_the_parameters_after_group_and_member_updates(B):
    shape, P, n = SHAPES["partial_block"], 2, 33
    g = group(B, shape, P)
    rows = rows_for(shape, P, n, np.float32)
    first = g.sample(rows)
    rings = []
    for i in range(P):
        rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=100 + i), (shape[0],), np.float32, (shape[1],), np.float32, device=0)
        rb.push(*transitions(shape, 40, 5 + i))
        rings.append(rb)
    g.opt(rings)                                        # no synchronisation in between: the acting launch is behind the round on the stream
    second = g.sample(rows)
    for i, m in enumerate(g.members):
        assert np.array_equal(second[i], own(m, rows[i], None)) and not np.array_equal(second[i], first[i]), i
    g.members[1].update_on_batch(*transitions(shape, BATCH, 9))
    third = g.sample(rows)
    assert np.array_equal(third[0], second[0]) and not np.array_equal(third[1], second[1])
    for i, m in enumerate(g.members):
        assert np.array_equal(third[i], own(m, rows[i], None)), i
    assert [m.n_opts for m in g.members] == [1, 2]
    g.opt(rings)                                        # acting went through no member's batch buffers: the round still steps
    g.sync()
    assert [m.n_opts for m in g.members] == [2, 3]
    g.close()
    for rb in rings: rb.close()
