"""BcGroup (csrc/bc_group.hpp through the C ABI) against its twins: the same configs built as standalone Bc agents with the same
initial parameters, stepped one after the other on rings holding the same rows with the same seeds.  Everything is compared bit for
bit (np.array_equal): a group round runs the bodies of the standalone kernels on the same arguments.

The shapes are the smallest at which each kernel can still go wrong:
  obs act units      act_out  B   what it reaches
  17  6   (64, 48)   None     7   one partial row block, padded widths
  45  24  (256, 256) Tanh     40  two row blocks with the last one partial: the per-member ticket and the loss's block order
  21  40  (64,)      Sigmoid  33  k_bc_head_mfma<2>, L = 2, no input-gradient launch in the head form
  9   4   ()         None     20  general only, L = 1: no input gradient at all
  21  65  (64, 40)   Tanh     50  general only, 128 padded output columns
11 rounds (more than the staging depth of 8, so slots are rewritten), round 5 an opt_with_record, and between rounds 6 and 7 one
member takes an update_on_batch of its own (member 1; member 0 in a group of one), as does its twin."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {
    "partial_block": (17, 6, (64, 48), "None", 7, ("general", "fused_mfma")),
    "two_blocks": (45, 24, (256, 256), "Tanh", 40, ("general", "fused_mfma")),
    "head_nt2": (21, 40, (64,), "Sigmoid", 33, ("general", "fused_mfma")),
    "no_hidden": (9, 4, (), "None", 20, ("general",)),
    "wide_out": (21, 65, (64, 40), "Tanh", 50, ("general",)),
}
CASES = [(n, f) for n, s in SHAPES.items() for f in s[5]]
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
ROUNDS, RECORD_ROUND, OWN_UPDATE_AFTER = 11, 5, 6
N_ROWS = 100


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def config(B, shape, form, i, action_type="Continuous", units=None):
    """member i: its own seed and learning rate; Adam for even members, AdamW with weight decay for odd ones"""
    od, ad, un, act_out, bsz, _ = shape
    lr = 1e-3 * (1 + 0.5 * i)
    opt = B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
    return B.BcConfig(obs_dim=od, act_dim=ad, policy_model_config=B.BcModelConfig(B.CandleMlpConfig(tuple(un if units is None else units), act_out), opt),
                      batch_size=bsz, action_type=action_type, device=0, seed=3 + i, kernel_form=form)


def rows(shape, seed, n=N_ROWS):
    od, ad = shape[0], shape[1]
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32),
            rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.random(n) < 0.1).astype(np.int8), np.zeros(n, np.int8))


def ring(B, shape, seed, data=None, per=False, fill=True):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=128, seed=seed, per_config=B.PerConfig() if per else None),
                              (shape[0],), np.float32, (shape[1],), np.float32, device=0)
    if fill:
        rb.push(*(data if data is not None else rows(shape, 1000 + seed)))
    return rb


def own_batch(shape, i):
    o, a = rows(shape, 5000 + i, shape[4])[:2]
    return o, a


def state(a, rb, shape):
    bsz = shape[4]
    return {**{r: a.get_params(role=r) for r in ROLES}, "n_opts": a.n_opts, "pred": a.probe("pred", bsz), "dz": a.probe("dz", bsz),
            "next_ixs": rb.sample_indices(8)}


def assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (tag, k)


def twins(B, shape, form, P, own):
    """the members' twins, one after the other: (state, recorded loss) per member"""
    out = []
    for i in range(P):
        a, rb = B.Bc.build(config(B, shape, form, i)), ring(B, shape, 100 + i)
        rec = None
        for k in range(1, ROUNDS + 1):
            if k == RECORD_ROUND: rec = a.opt_with_record(rb)
            else: a.opt(rb)
            if k == OWN_UPDATE_AFTER and i == own: a.update_on_batch(*own_batch(shape, i))
        a.sync()
        out.append((state(a, rb, shape), rec["loss"]))
        a.close(); rb.close()
    return out


@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("name,form", CASES)
def test_the_group_equals_its_twins_bit_for_bit(B, name, form, P):
    shape = SHAPES[name]
    own = min(1, P - 1)
    want = twins(B, shape, form, P, own)
    g = B.BcGroup.build([config(B, shape, form, i) for i in range(P)])
    rings = [ring(B, shape, 100 + i) for i in range(P)]
    L = len(shape[2]) + 1
    count = 2 * L + 4 if form == "general" else 2 * L + 2
    assert len(g) == P and g.form == "bc_layers" and g.launches_per_round == count and g.kernel_launches == 0
    recs = None
    for k in range(1, ROUNDS + 1):
        if k == RECORD_ROUND: recs = g.opt_with_record()
        else: g.opt(rings if k == 1 else None)
        if k == OWN_UPDATE_AFTER: g.members[own].update_on_batch(*own_batch(shape, own))
    g.sync()
    assert g.kernel_launches == ROUNDS * count
    for i, (m, rb) in enumerate(zip(g.members, rings)):
        assert_same(state(m, rb, shape), want[i][0], (name, form, P, i))
        assert np.float32(recs[i]["loss"]) == np.float32(want[i][1]), (name, form, P, i, recs[i], want[i][1])
        assert m.n_opts == ROUNDS + (1 if i == own else 0)
    g.close()
    for rb in rings: rb.close()


def test_members_stay_ordinary_agents_after_adoption(B):
    """one update_on_batch on a member right after the group's opt: the member's own call, on the group's stream"""
    shape = SHAPES["partial_block"]
    g = B.BcGroup.build([config(B, shape, "general", i) for i in range(2)])
    rings = [ring(B, shape, 100 + i) for i in range(2)]
    g.opt(rings)
    rec = g.members[1].update_on_batch(*own_batch(shape, 1))
    got = state(g.members[1], rings[1], shape)
    a, rb = B.Bc.build(config(B, shape, "general", 1)), ring(B, shape, 101)
    a.opt(rb)
    want_rec = a.update_on_batch(*own_batch(shape, 1))
    assert_same(got, state(a, rb, shape), "adoption")
    assert np.float32(rec["loss"]) == np.float32(want_rec["loss"])
    a.close(); rb.close(); g.close()
    for r in rings: r.close()


@pytest.mark.parametrize("what", ["second_shape", "fused", "discrete"])
def test_a_member_that_cannot_join_is_named_and_nobody_is_adopted(B, what):
    shape = SHAPES["partial_block"]
    bad = {"second_shape": lambda: config(B, shape, "general", 1, units=(64, 64)),
           "fused": lambda: config(B, shape, "fused", 1),
           "discrete": lambda: config(B, shape, "general", 1, action_type="Discrete")}[what]()
    agents = [B.Bc.build(config(B, shape, "general", 0)), B.Bc.build(bad)]
    with pytest.raises(B.BdrError, match="member 1"):
        B.BcGroup(agents)
    # nothing moved: member 0 is still a standalone agent and steps as its twin does
    rb = ring(B, shape, 100)
    for _ in range(2): agents[0].opt(rb)
    got = state(agents[0], rb, shape)
    a, rb2 = B.Bc.build(config(B, shape, "general", 0)), ring(B, shape, 100)
    for _ in range(2): a.opt(rb2)
    assert_same(got, state(a, rb2, shape), what)
    for x in agents + [a]: x.close()
    rb.close(); rb2.close()


def test_refused_buffers_name_the_member_and_move_nothing(B):
    shape = SHAPES["partial_block"]
    g = B.BcGroup.build([config(B, shape, "general", i) for i in range(2)])
    rings = [ring(B, shape, 100 + i) for i in range(2)]
    per, empty = ring(B, shape, 7, per=True), ring(B, shape, 8, fill=False)
    for bad in ([rings[0], per], [rings[0], empty], [rings[0], rings[0]]):
        with pytest.raises(B.BdrError, match="member 1"):
            g.opt(bad)
        with pytest.raises(B.BdrError, match="member 1"):
            g.opt_with_record(bad)
    with pytest.raises(ValueError):
        g.opt([rings[0]])
    with pytest.raises(B.BdrError, match="group"):
        g.members[0].close()
    assert g.kernel_launches == 0
    for _ in range(2): g.opt(rings)
    g.sync()
    for i in range(2):
        a, rb = B.Bc.build(config(B, shape, "general", i)), ring(B, shape, 100 + i)
        for _ in range(2): a.opt(rb)
        a.sync()
        assert_same(state(g.members[i], rings[i], shape), state(a, rb, shape), i)
        a.close(); rb.close()
    g.close()
    for r in rings + [per, empty]: r.close()


def test_train_offline_is_a_loop_over_opt_and_opt_with_record(B):
    shape = SHAPES["partial_block"]
    g = B.BcGroup.build([config(B, shape, "fused_mfma", i) for i in range(2)])
    rings = [ring(B, shape, 100 + i) for i in range(2)]
    seen = []
    g.train_offline(rings, 4, record_interval=2, on_record=lambda k, recs: seen.append((k, [np.float32(r["loss"]) for r in recs])))
    assert [k for k, _ in seen] == [2, 4] and g.kernel_launches == 4 * g.launches_per_round
    for i in range(2):
        a, rb = B.Bc.build(config(B, shape, "fused_mfma", i)), ring(B, shape, 100 + i)
        losses = [np.float32(a.opt_with_record(rb)["loss"]) if k % 2 == 0 else a.opt(rb) for k in range(1, 5)]
        a.sync()
        assert [seen[0][1][i], seen[1][1][i]] == [losses[1], losses[3]]
        assert_same(state(g.members[i], rings[i], shape), state(a, rb, shape), i)
        a.close(); rb.close()
    g.close()
    for r in rings: r.close()


# the smallest shape the host path of a round needs: obs 4, act 2, one hidden layer of 64, B = 33 (two row blocks, the last partial)
TINY = (4, 2, (64,), "None", 33, ("general",))


def test_a_buffer_closed_since_the_last_opt_and_a_null_buffer_are_refused_and_move_nothing(B):
    """opt() without buffers steps on the buffers named last: one closed since is refused here, naming the member, before the library
    sees its stale handle; a None buffer is the library's own refusal, not an AttributeError"""
    g = B.BcGroup.build([config(B, TINY, "general", i) for i in range(2)])
    rings = [ring(B, TINY, 100 + i) for i in range(2)]
    g.opt(rings)
    g.sync()
    moved = lambda: [{r: m.get_params(role=r) for r in ROLES} for m in g.members]
    before, launches = moved(), g.kernel_launches
    rings[1].close()
    for call in (g.opt, g.opt_with_record):
        with pytest.raises(ValueError, match="member 1"):
            call()
    with pytest.raises(B.BdrError, match="member 0: null buffer"):
        g.opt([None, rings[0]])
    g.sync()
    assert g.kernel_launches == launches and [m.n_opts for m in g.members] == [1, 1]
    for got, want in zip(moved(), before):
        assert_same(got, want, "closed buffer")
    g.close()
    rings[0].close()
