"""BcGroup.sample (csrc/bc_group.hpp k_bc_act_group through the C ABI): every selected member gets the bits of its own
bdr_agent_sample_raw, on the layer path and on the one-launch path (np.array_equal on the raw bits throughout).

The shapes are the smallest at which the kernel can still go wrong (the first five are those of tests/test_gpu_bc_group.py):
  obs act units      act_out  what it reaches
  17  6   (64, 48)   None     padded widths
  45  24  (256, 256) Tanh     the prefetch across layers with Kp = 256, two teams
  9   4   ()         None     one layer: no next-layer prefetch
  21  65  (64, 40)   Tanh     128 padded output columns, A not a multiple of 32
  9   4   (300,)     None     Kp = 320 > 256: the in-tile weight loads
  9   4   (480,)     None     W = 480 > 448: the one-team entry k_bc_act_group<1>
with P = 1, 2, 5 members and n = 1, 32, 33 rows: one block, a full block, two blocks with one row in the second."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {
    "padded": (17, 6, (64, 48), "None"),
    "two_teams_k256": (45, 24, (256, 256), "Tanh"),
    "one_layer": (9, 4, (), "None"),
    "wide_out": (21, 65, (64, 40), "Tanh"),
    "k320": (9, 4, (300,), "None"),
    "one_team": (9, 4, (480,), "None"),
}
NS = (1, 32, 33)
SENTINEL = np.float32(-7777.25)


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def config(B, shape, i, bsz=8):
    od, ad, un, act_out = shape
    lr = 1e-3 * (1 + 0.5 * i)
    opt = B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
    return B.BcConfig(obs_dim=od, act_dim=ad, policy_model_config=B.BcModelConfig(B.CandleMlpConfig(tuple(un), act_out), opt),
                      batch_size=bsz, action_type="Continuous", device=0, seed=3 + i, kernel_form="general")


def group(B, shape, P):
    return B.BcGroup.build([config(B, shape, i) for i in range(P)])


def normaliser(B, O, seed=0):
    rng = np.random.default_rng(900 + seed)
    return B.ObsNormalizer(O, 0).set(rng.standard_normal(O).astype(np.float32), rng.uniform(0.5, 2.0, O).astype(np.float32))


def rows_for(shape, P, n, dtype, seed=0):
    rng = np.random.default_rng(77 + seed)
    return [(3.0 * rng.standard_normal((n, shape[0]))).astype(dtype) for _ in range(P)]


def own(member, rows, norm):
    """the member's own bdr_agent_sample_raw on both act paths: one result, the two paths hold the same bits"""
    out = []
    for path in ("layers", "fused"):
        member.set_act_path(path)
        out.append(member.sample_raw(rows, norm))
    member.set_act_path("default")
    assert np.array_equal(out[0], out[1])
    return out[0]


@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("name", list(SHAPES))
def test_group_sample_equals_each_members_own_sample_raw(B, name, P):
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
    """bdr_bc_group_sample_members as the C caller sees it: every array indexed by member"""
    from border_amd import _lib
    P = len(g)
    ptr = lambda a: None if a is None else a.ctypes.data
    rp, op = (C.c_void_p * P)(*[ptr(r) for r in rows]), (C.c_void_p * P)(*[ptr(o) for o in outs])
    cp = (C.c_int32 * P)(*codes)
    np_ = None if norms is None else (C.c_void_p * P)(*[None if z is None else z.handle for z in norms])
    if members is None:
        return _lib.lib().bdr_bc_group_sample(g.handle, np_, n, rp, cp, op)
    sel = np.asarray(members, np.uint32)
    return _lib.lib().bdr_bc_group_sample_members(g.handle, sel.ctypes.data_as(C.c_void_p), sel.size, np_, n, rp, cp, op)


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
    # the Python method: one entry per member, None for those that did not act; unselected members need no rows
    got = g.sample([rows[0], None, None, rows[3], None], members=[0, 3])
    assert [x is None for x in got] == [False, True, True, False, True] and np.array_equal(got[3], outs[3])
    # with every member selected the second call gives what the first gives
    all_a, all_b = g.sample(rows), g.sample(rows, members=list(range(P)))
    assert all(np.array_equal(a, b) for a, b in zip(all_a, all_b))
    g.close()


def test_two_members_on_one_host_pointer(B):
    shape, P, n = SHAPES["wide_out"], 2, 32
    g = group(B, shape, P)
    x = rows_for(shape, 1, n, np.float64)[0]
    got = g.sample(x)                                   # one array for all members: an ensemble on one observation batch
    outs = [np.full((n, shape[1]), SENTINEL, np.float32) for _ in range(P)]
    assert raw_call(B, g, None, n, [x, x], [1, 1], outs) == 0
    for i, m in enumerate(g.members):
        want = own(m, x, None)
        assert np.array_equal(got[i], want) and np.array_equal(outs[i], want), i
    assert not np.array_equal(got[0], got[1])           # two members, two parameter sets
    g.close()


def test_actions_follow_the_parameters_after_group_and_member_updates(B):
    shape, P, n = SHAPES["padded"], 2, 33
    od, ad = shape[0], shape[1]
    g = group(B, shape, P)
    rows = rows_for(shape, P, n, np.float32)
    first = g.sample(rows)
    rng = np.random.default_rng(5)
    rings = []
    for i in range(P):
        rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=100 + i), (od,), np.float32, (ad,), np.float32, device=0)
        rb.push(rng.standard_normal((40, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (40, ad)).astype(np.float32),
                rng.standard_normal((40, od)).astype(np.float32), np.zeros(40, np.float32), np.zeros(40, np.int8), np.zeros(40, np.int8))
        rings.append(rb)
    g.opt(rings)                                        # no synchronisation in between: the acting launch is behind the round on the stream
    second = g.sample(rows)
    for i, m in enumerate(g.members):
        assert np.array_equal(second[i], own(m, rows[i], None)) and not np.array_equal(second[i], first[i]), i
    g.members[1].update_on_batch(rng.standard_normal((8, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (8, ad)).astype(np.float32))
    third = g.sample(rows)
    assert np.array_equal(third[0], second[0]) and not np.array_equal(third[1], second[1])
    for i, m in enumerate(g.members):
        assert np.array_equal(third[i], own(m, rows[i], None)), i
    assert [m.n_opts for m in g.members] == [1, 2]
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


def test_every_refusal_names_the_member_and_writes_nothing(B):
    from border_amd import _lib
    shape, P, n = SHAPES["padded"], 5, 2
    g = group(B, shape, P)
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
    assert np.array_equal(outs[4], own(g.members[4], rows[4], None)) and np.all(outs[0] == SENTINEL)
    g.close(); unfinished.close(); other.close()
    # a network wider than the kernel's LDS plan: refused, naming the member; the member keeps acting standalone
    wide = (9, 4, (600,), "None")
    g = group(B, wide, 2)
    rows, outs = rows_for(wide, 2, n, np.float32), [np.full((n, 4), SENTINEL, np.float32) for _ in range(2)]
    assert raw_call(B, g, [1], n, rows, [0, 0], outs) == 1
    msg = _lib.lib().bdr_last_error().decode()
    assert "member 1" in msg and "standalone" in msg and np.all(outs[1] == SENTINEL), msg
    assert g.members[1].sample_raw(rows[1]).shape == (n, 4)
    g.close()
    # 3 x 65536 x 45 x 8 bytes of float64 rows are past the 64 MiB of one call: refused before a byte is read (the arrays here are small)
    big = SHAPES["two_teams_k256"]
    g = group(B, big, 3)
    rows, outs = rows_for(big, 3, n, np.float64), [np.full((n, big[1]), SENTINEL, np.float32) for _ in range(3)]
    assert raw_call(B, g, None, 65536, rows, [1, 1, 1], outs) == 1
    msg = _lib.lib().bdr_last_error().decode()
    assert "split" in msg and "member 0" in msg and all(np.all(o == SENTINEL) for o in outs) and g.kernel_launches == 0, msg
    g.close()
