"""IqlGroup.sample (csrc/candle_act_group.hpp k_candle_act_group through the C ABI): every selected member gets the bits of its own
bdr_agent_sample_raw in the mode it is in, at the noise counter it is at (np.array_equal on the raw bits throughout).

In eval mode a member's own call moves nothing, so the group is compared against the members themselves, on the layer path and on the
one-launch path.  In train mode every call takes draws, so the group is compared against TWINS: standalone Iql agents built from the
same configs, which make the standalone calls of exactly the calls their member took part in.

Shapes (obs, act, actor units; value and critic are (64,), two critics), the smallest at which the kernel can still go wrong:
  17  6   (64, 48)     padded widths
  45  24  (256, 256)   the prefetch across layers with Kp = 256, two teams
  9   4   (64,)        the shallowest actor IQL admits
  21  65  (64, 40)     128 padded output columns, A not a multiple of 32
  9   4   (300,)       Kp = 320 > 256: the in-tile weight loads
  9   4   (480,)       W = 480 > 448: the one-team entry k_candle_act_group<1>
with P = 1, 2, 5 members and n = 1, 32, 33 rows: one block, a full block, two blocks with one row in the second.  Member i differs from
member 0 in seed, action limit (Clamp with its own bounds for even i, Tanh with its own scale for odd i) and the log-std clamps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {
    "padded": (17, 6, (64, 48)),
    "two_teams_k256": (45, 24, (256, 256)),
    "shallow": (9, 4, (64,)),
    "wide_out": (21, 65, (64, 40)),
    "k320": (9, 4, (300,)),
    "one_team": (9, 4, (480,)),
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
    from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, IqlConfig, MultiCriticConfig, ValueConfig
    od, ad, un = shape
    opt = lambda: B.OptimizerConfig.Adam(1e-3 * (1 + 0.5 * i))
    limit = ActionLimit.Tanh(1.0 + 0.25 * i) if i % 2 else ActionLimit.Clamp(-0.5 - 0.1 * i, 0.6 + 0.1 * i)
    lo, hi = log_std if log_std is not None else (-3.0 + 0.5 * i, 1.0 - 0.2 * i)
    return IqlConfig(obs_dim=od, act_dim=ad, value_config=ValueConfig(CandleMlpConfig((64,)), opt()),
                     critic_config=MultiCriticConfig(2, CandleMlpConfig((64,)), opt(), 0.005),
                     actor_config=GaussianActorConfig(CandleMlpConfig(tuple(un)), opt(), min_log_std=lo, max_log_std=hi, action_limit=limit),
                     batch_size=BATCH, seed=3 + i, device=0)


def group(B, shape, P, **kw):
    return B.IqlGroup.build([config(B, shape, i, **kw) for i in range(P)])


def twins(B, shape, P, **kw):
    return [B.Iql.build(config(B, shape, i, **kw)) for i in range(P)]


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


def test_the_three_branches_of_the_log_std_clamp(B):
    shape, P, n = SHAPES["padded"], 3, 33
    A = shape[1]
    clamps = [(0.5, 2.0), (-20.0, -0.5), (-20.0, 2.0)]                       # above head2, below head2, around head2
    head2 = np.linspace(-0.3, 0.3, A).astype(np.float32)
    cfgs = [config(B, shape, i, log_std=clamps[i]) for i in range(P)]
    g, tw = B.IqlGroup.build(cfgs), [B.Iql.build(c) for c in cfgs]
    for a in g.members + tw:
        p = a.get_params("actor")
        p[-A:] = head2
        a.set_params(p, "actor")
        a.train()
    h = [m.get_params("actor")[-A:] for m in g.members]                      # through the parameter view: head2 as the kernel reads it
    assert np.all(np.float32(clamps[0][0]) > h[0])                           # min_log_std above every head2 value: the lower clamp acts
    assert np.all(np.float32(clamps[1][1]) < h[1])                           # max_log_std below every value: the upper clamp acts
    assert np.all((np.float32(clamps[2][0]) < h[2]) & (h[2] < np.float32(clamps[2][1])))   # clamps that contain them: head2 itself
    rows = rows_for(shape, P, n, np.float32)
    got = g.sample(rows)
    for i in range(P):
        assert np.array_equal(got[i], twin_call(tw[i], rows[i])), i
    for m in g.members: m.eval()
    mean = g.sample(rows)
    assert all(not np.array_equal(mean[i], got[i]) for i in range(P))        # the draws were applied
    g.close()
    for t in tw: t.close()


def test_members_with_different_dtypes_and_normalisers_in_one_call(B):
    shape, P, n = SHAPES["two_teams_k256"], 5, 33
    g = group(B, shape, P)
    nzs = [normaliser(B, shape[0], 1), None, normaliser(B, shape[0], 2), None, None]
    rows = [rows_for(shape, 1, n, np.float64 if i % 2 else np.float32, seed=i)[0] for i in range(P)]
    got = g.sample(rows, nzs)
    for i, m in enumerate(g.members):
        assert np.array_equal(got[i], own(m, rows[i], nzs[i])), i
    g.close()
    for z in nzs:
        if z is not None: z.close()


def raw_call(B, g, members, n, rows, codes, outs, norms=None):
    """bdr_iql_group_sample_members as the C caller sees it: every array indexed by member"""
    from border_amd import _lib
    P = len(g)
    ptr = lambda a: None if a is None else a.ctypes.data
    rp, op = (C.c_void_p * P)(*[ptr(r) for r in rows]), (C.c_void_p * P)(*[ptr(o) for o in outs])
    cp = (C.c_int32 * P)(*codes)
    np_ = None if norms is None else (C.c_void_p * P)(*[None if z is None else z.handle for z in norms])
    if members is None:
        return _lib.lib().bdr_iql_group_sample(g.handle, np_, n, rp, cp, op)
    sel = np.asarray(members, np.uint32)
    return _lib.lib().bdr_iql_group_sample_members(g.handle, sel.ctypes.data_as(C.c_void_p), sel.size, np_, n, rp, cp, op)


def test_a_subset_selection_leaves_the_other_members_untouched(B):
    shape, P, n = SHAPES["padded"], 5, 33
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


def test_two_members_on_one_host_pointer(B):
    shape, P, n = SHAPES["wide_out"], 2, 32
    g = group(B, shape, P)
    x = rows_for(shape, 1, n, np.float64)[0]
    got = g.sample(x)
    outs = [np.full((n, shape[1]), SENTINEL, np.float32) for _ in range(P)]
    assert raw_call(B, g, None, n, [x, x], [1, 1], outs) == 0
    for i, m in enumerate(g.members):
        want = own(m, x, None)
        assert np.array_equal(got[i], want) and np.array_equal(outs[i], want), i
    assert not np.array_equal(got[0], got[1])
    g.close()


def transitions(shape, n, seed):
    od, ad = shape[0], shape[1]
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32),
            rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal(n).astype(np.float32), np.zeros(n, np.int8), np.zeros(n, np.int8))


def test_actions_follow_the_parameters_after_group_and_member_updates(B):
    shape, P, n = SHAPES["padded"], 2, 33
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


def test_a_call_larger_than_the_staging_area_then_a_smaller_one(B):
    shape, P = SHAPES["padded"], 2
    g = group(B, shape, P)
    small = rows_for(shape, P, 1, np.float64)
    a = g.sample(small)                                 # the first call sizes the areas: 64 KiB of rows, 16 Ki floats of actions
    big = rows_for(shape, P, 3000, np.float64, seed=1)  # 2 x 3000 x 17 x 8 bytes of rows, 2 x 3000 x 6 floats of actions: both grow
    b = g.sample(big)
    c = g.sample(small)
    for i, m in enumerate(g.members):
        m.set_act_path("fused")
        assert np.array_equal(b[i], m.sample_raw(big[i])), i
        assert np.array_equal(a[i], c[i]) and np.array_equal(c[i], m.sample_raw(small[i])), i
    g.close()


def test_every_refusal_names_the_member_writes_nothing_and_moves_no_counter(B):
    from border_amd import _lib
    shape, P, n = SHAPES["padded"], 5, 2
    g, tw = group(B, shape, P), twins(B, shape, P)
    for a in g.members + tw: a.train()
    rows = rows_for(shape, P, n, np.float32)
    outs = [np.full((n, shape[1]), SENTINEL, np.float32) for _ in range(P)]
    unfinished, other = B.ObsNormalizer(shape[0], 0), normaliser(B, shape[0] + 1)
    ok = [0] * P

    def refused(match, members, rows_=rows, codes=ok, outs_=outs, norms=None, n_=n):
        before = g.kernel_launches
        assert raw_call(B, g, members, n_, rows_, codes, outs_, norms) == 1      # BDR_ERR_INVALID
        msg = _lib.lib().bdr_last_error().decode()
        assert match in msg, msg
        assert g.kernel_launches == before and all(np.all(o == SENTINEL) for o in outs if o is not None)
        got = g.sample(rows)                     # a train-mode call still equals the twins, which never saw the refused call
        for i in range(P):
            assert np.array_equal(got[i], twin_call(tw[i], rows[i])), (match, i)

    refused("member 3", [0, 3], rows_=rows[:3] + [None] + rows[4:])                    # null rows of a selected member
    refused("member 3", [0, 3], outs_=outs[:3] + [None] + outs[4:])                    # null output of a selected member
    refused("empty", [])
    refused("member 1", [2, 1])                                                        # not strictly ascending
    refused("member 2", [2, 2])
    refused("member 5", [0, 5])                                                        # out of range
    refused("member 2", [0, 2], norms=[None, None, unfinished, None, None])            # a normaliser without statistics
    refused("member 4", None, norms=[None, None, None, None, other])                   # another dim
    refused("member 1", None, codes=[0, 9, 0, 0, 0])                                   # an unknown dtype
    refused("batch size", None, n_=0)
    refused("batch size", None, n_=65537)
    # a selection that names only good members is served although other members' entries are bad
    assert raw_call(B, g, [1, 4], n, [None, rows[1], None, None, rows[4]], [7, 0, 7, 7, 0], [None, outs[1], None, None, outs[4]]) == 0
    assert np.array_equal(outs[4], twin_call(tw[4], rows[4])) and np.array_equal(outs[1], twin_call(tw[1], rows[1])) and np.all(outs[0] == SENTINEL)
    g.close(); unfinished.close(); other.close()
    for t in tw: t.close()
    # an actor wider than the kernel's LDS plan: the group is created and steps; acting is refused at the first call, naming the member,
    # and the member keeps acting standalone
    wide = (9, 4, (600,))
    g = group(B, wide, 2)
    rows, outs = rows_for(wide, 2, n, np.float32), [np.full((n, 4), SENTINEL, np.float32) for _ in range(2)]
    for m in g.members: m.train()
    assert raw_call(B, g, [1], n, rows, [0, 0], outs) == 1
    msg = _lib.lib().bdr_last_error().decode()
    assert "member 1" in msg and "standalone" in msg and np.all(outs[1] == SENTINEL), msg
    t = B.Iql.build(config(B, wide, 1)); t.train()
    assert np.array_equal(g.members[1].sample_raw(rows[1]), t.sample_raw(rows[1]))     # the refused call took no draw
    g.close(); t.close()
    # 3 x 65536 x 45 x 8 bytes of float64 rows are past the 64 MiB of one call: refused before a byte is read (the arrays here are small)
    big = SHAPES["two_teams_k256"]
    g = group(B, big, 3)
    rows, outs = rows_for(big, 3, n, np.float64), [np.full((n, big[1]), SENTINEL, np.float32) for _ in range(3)]
    assert raw_call(B, g, None, 65536, rows, [1, 1, 1], outs) == 1
    msg = _lib.lib().bdr_last_error().decode()
    assert "split" in msg and "member 0" in msg and all(np.all(o == SENTINEL) for o in outs) and g.kernel_launches == 0, msg
    g.close()
