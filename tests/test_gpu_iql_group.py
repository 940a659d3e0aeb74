"""IqlGroup (csrc/iql_group.hpp through the C ABI) against its twins: the same configs built as standalone Iql agents, stepped one after
the other on rings holding the same rows with the same seeds.  Everything is compared bit for bit (np.array_equal): a group round runs
the bodies of the standalone kernels on the same arguments.

Rings have capacity 128 and hold 100 random rows, `term` at rate 0.1.  The shapes are the smallest at which a kernel can still go wrong:
  obs act  value / critic / actor units            NC  B   what it reaches
  17  6    (64,48) / (64,48) / (64,48)             2   7   one partial row block, padded widths, z = 4 forward
  45  24   (256,256) all, Tanh, SmoothL1, softmax  2   40  two row blocks with the last partial, Kq = 128, the batch-wide max / sum of the
                                                           actor loss per member
  9   4    () / () / (64,), value + critic ReLU    1   33  L = 1 networks (no dX launch), relu_out masks, z = 2 forward, one-instance track
  21  40   (64,) / (64,64,64) / (128,)             2   20  networks of unequal depth: the plan's per-network launch indexing
11 rounds (more than the staging depth of 8, so slots are rewritten), round 5 an opt_with_record, and after round 6 one member takes
an update_on_batch of its own (member 1; member 0 in a group of one), as does its twin.  Member i differs from member 0 in seed,
tau_iql, inv_lambda, gamma, critic_tau, exp_adv_max, the three learning rates, and Adam (even) against AdamW with weight decay (odd).
A twin depends on its index and on whether it takes the own update, not on P: each is computed once and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# obs, act, value units, critic units, actor units, value / critic activation_out, NC, B, (action limit, critic loss, adv_softmax)
SHAPES = {
    "partial_block": (17, 6, (64, 48), (64, 48), (64, 48), "None", 2, 7, ("Clamp", "Mse", False)),
    "two_blocks": (45, 24, (256, 256), (256, 256), (256, 256), "None", 2, 40, ("Tanh", "SmoothL1", True)),
    "no_hidden": (9, 4, (), (), (64,), "ReLU", 1, 33, ("Clamp", "Mse", False)),
    "unequal": (21, 40, (64,), (64, 64, 64), (128,), "None", 2, 20, ("Clamp", "Mse", False)),
}
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
PROBES = ("q_tgt_min_value", "v", "u", "tgt", "q_pred", "q_tgt_min_actor", "w", "logp", "v_next", "v_obs")
KEYS = ("loss_value", "loss_critic", "loss_actor")
ROUNDS, RECORD_ROUND, OWN_UPDATE_AFTER = 11, 5, 6
N_ROWS = 100


def lib():
    import border_amd
    return border_amd


@pytest.fixture(scope="module")
def B():
    border_amd = lib()
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def launch_count(shape):
    Lv, Lq, Lp = len(shape[2]) + 1, len(shape[3]) + 1, len(shape[4]) + 1
    return 3 * (Lq + Lv) + 2 * Lp + 8


def config(B, shape, i, mixed=False, **kw):
    """member i: everything the group leaves free differs from member 0's; mixed: adv_softmax, critic_loss and the action limit vary too"""
    od, ad, vu, qu, pu, act_out, nc, bsz, (limit, closs, softmax) = shape
    if mixed:
        limit, closs, softmax = ("Clamp", "Tanh", "Clamp")[i % 3], ("Mse", "SmoothL1")[i % 2], bool((i // 2) % 2 == 0 and i > 0)

    def opt(lr):
        return B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
    from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, IqlConfig, MultiCriticConfig, ValueConfig
    c = IqlConfig(obs_dim=od, act_dim=ad,
                  value_config=ValueConfig(CandleMlpConfig(tuple(vu), act_out), opt(1e-3 * (1 + 0.5 * i))),
                  critic_config=MultiCriticConfig(nc, CandleMlpConfig(tuple(qu), act_out), opt(2e-3 * (1 + 0.25 * i)), 0.005 * (1 + i)),
                  actor_config=GaussianActorConfig(CandleMlpConfig(tuple(pu), "None"), opt(5e-4 * (1 + i)),
                                                   action_limit=ActionLimit.Tanh(1.0) if limit == "Tanh" else ActionLimit.Clamp()),
                  gamma=0.99 - 0.02 * i, tau_iql=0.7 + 0.04 * i, inv_lambda=3.0 / (1 + i), exp_adv_max=100.0 / (1 + 3 * i), batch_size=bsz,
                  adv_softmax=softmax, critic_loss=closs, seed=3 + i, device=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


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
    return rows(shape, 5000 + i, shape[7])


def models(shape):
    nc = shape[6]
    return ["actor", "value"] + [f"critic_{i}" for i in range(nc)], [f"critic_tgt_{i}" for i in range(nc)]


def state(a, rb, shape):
    bsz = shape[7]
    trained, targets = models(shape)
    out = {(m, r): a.get_params(m, role=r) for m in trained for r in ROLES}
    out.update({(m, "param"): a.get_params(m) for m in targets})
    out.update({("probe", p): a.probe(p, bsz) for p in PROBES})
    out["n_opts"] = a.n_opts
    out["next_ixs"] = rb.sample_indices(8)
    return out


def assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (tag, k)


def rec_bits(rec):
    return [np.float32(rec[k]).view(np.uint32) for k in KEYS]


@functools.lru_cache(maxsize=None)
def twin(name, i, own, mixed=False):
    """member i's twin, stepped alone: (state, the record of round 5)"""
    B, shape = lib(), SHAPES[name]
    a, rb = B.Iql.build(config(B, shape, i, mixed)), ring(B, shape, 100 + i)
    rec = None
    for k in range(1, ROUNDS + 1):
        if k == RECORD_ROUND: rec = a.opt_with_record(rb)
        else: a.opt(rb)
        if k == OWN_UPDATE_AFTER and own: a.update_on_batch(*own_batch(shape, i))
    a.sync()
    out = (state(a, rb, shape), rec)
    a.close(); rb.close()
    return out


def run_group(B, name, P, mixed=False):
    shape = SHAPES[name]
    own = min(1, P - 1)
    g = B.IqlGroup.build([config(B, shape, i, mixed) for i in range(P)])
    rings = [ring(B, shape, 100 + i) for i in range(P)]
    count = launch_count(shape)
    assert len(g) == P and g.form == "iql_layers" and g.launches_per_round == count and g.kernel_launches == 0
    recs = None
    for k in range(1, ROUNDS + 1):
        if k == RECORD_ROUND: recs = g.opt_with_record()
        else: g.opt(rings if k == 1 else None)
        if k == OWN_UPDATE_AFTER: g.members[own].update_on_batch(*own_batch(shape, own))
    g.sync()
    assert g.kernel_launches == ROUNDS * count
    for i, (m, rb) in enumerate(zip(g.members, rings)):
        want, want_rec = twin(name, i, i == own, mixed)
        assert_same(state(m, rb, shape), want, (name, P, i))
        assert list(recs[i]) == list(KEYS) and rec_bits(recs[i]) == rec_bits(want_rec), (name, P, i, recs[i], want_rec)
        assert m.n_opts == ROUNDS + (1 if i == own else 0)
    g.close()
    for rb in rings: rb.close()


@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_group_equals_its_twins_bit_for_bit(B, name, P):
    run_group(B, name, P)


def test_members_may_mix_adv_softmax_critic_loss_and_action_limit(B):
    cfgs = [config(B, SHAPES["partial_block"], i, True) for i in range(5)]
    assert len({c.adv_softmax for c in cfgs}) == 2 and len({c.critic_loss for c in cfgs}) == 2
    assert len({c.actor_config.action_limit.kind for c in cfgs}) == 2
    run_group(B, "partial_block", 5, mixed=True)


def test_a_group_over_views_of_one_ring_equals_its_twins_on_three_rings(B):
    shape = SHAPES["partial_block"]
    data = rows(shape, 21)
    owner = ring(B, shape, 99, data)
    views = [owner.view(50 + i) for i in range(3)]
    g = B.IqlGroup.build([config(B, shape, i) for i in range(3)])
    g.opt(views)
    recs = g.opt_with_record()
    g.opt()
    g.sync()
    for i in range(3):
        a, rb = B.Iql.build(config(B, shape, i)), ring(B, shape, 50 + i, data)
        a.opt(rb)
        rec = a.opt_with_record(rb)
        a.opt(rb)
        a.sync()
        assert_same(state(g.members[i], views[i], shape), state(a, rb, shape), ("views", i))
        assert rec_bits(recs[i]) == rec_bits(rec)
        a.close(); rb.close()
    g.close()
    for v in views: v.close()
    owner.close()


def stepped_alone(B, shape, i, n):
    a, rb = B.Iql.build(config(B, shape, i)), ring(B, shape, 100 + i)
    for _ in range(n): a.opt(rb)
    a.sync()
    out = state(a, rb, shape)
    a.close(); rb.close()
    return out


@pytest.mark.parametrize("what", ["second_shape", "three_critics", "two_updates", "not_iql", "twice"])
def test_a_member_that_cannot_join_is_named_and_nobody_is_adopted(B, what):
    shape = SHAPES["partial_block"]
    first = B.Iql.build(config(B, shape, 0))
    if what == "second_shape":
        bad = B.Iql.build(config(B, SHAPES["unequal"], 1, batch_size=shape[7]))
    elif what == "three_critics":
        c = config(B, shape, 1)
        c.critic_config.n_nets = 3
        bad = B.Iql.build(c)
    elif what == "two_updates":
        bad = B.Iql.build(config(B, shape, 1, n_updates_per_opt=2))
    elif what == "not_iql":
        bad = B.Bc.build(B.BcConfig(obs_dim=shape[0], act_dim=shape[1], policy_model_config=B.BcModelConfig(B.CandleMlpConfig((64,), "None"), B.OptimizerConfig.Adam(1e-3)),
                                    batch_size=shape[7], action_type="Continuous", device=0, seed=1))
    else:
        bad = first
    with pytest.raises(B.BdrError, match="member 1"):
        B.IqlGroup([first, bad])
    # nothing moved: member 0 is still a standalone agent and steps as its twin does
    rb = ring(B, shape, 100)
    for _ in range(2): first.opt(rb)
    first.sync()
    assert_same(state(first, rb, shape), stepped_alone(B, shape, 0, 2), what)
    first.close(); rb.close()
    if bad is not first: bad.close()


# observation rows of 16 bytes: the width a single-frame store of one frame can have
STORE_SHAPE = (4, 6, (64, 48), (64, 48), (64, 48), "None", 2, 7, ("Clamp", "Mse", False))


def test_refused_buffers_name_the_member_and_move_nothing(B):
    """every buffer rule of a grouped opt, with member 1 the one concerned: member 0 has a good ring, so a check made only once the
    round is under way would have moved member 0's step counters, n_opts and stream position before it refused"""
    shape = STORE_SHAPE
    cfg = lambda **kw: B.SimpleReplayBufferConfig(capacity=128, **kw)
    g = B.IqlGroup.build([config(B, shape, i) for i in range(2)])
    rings = [ring(B, shape, 100 + i) for i in range(2)]
    per, empty = ring(B, shape, 7, per=True), ring(B, shape, 8, fill=False)
    other = B.SimpleReplayBuffer(cfg(seed=9), (shape[0] + 1,), np.float32, (shape[1],), np.float32, device=0)
    other.push(*rows((shape[0] + 1, shape[1]), 3))
    xoshiro = B.SimpleReplayBuffer(cfg(seed=10, index_rng="xoshiro256++"), (shape[0],), np.float32, (shape[1],), np.float32, device=0)
    xoshiro.push(*rows(shape, 4))
    store = B.SimpleReplayBuffer(cfg(seed=11, frame_stack=1), (shape[0],), np.float32, (shape[1],), np.float32, device=0)
    cases = {"prioritized": per, "empty": empty, "shares": rings[0], "null buffer": None, "do not match": other, "StdRng": xoshiro, "single-frame": store}
    for word, wrong in cases.items():
        for call in (g.opt, g.opt_with_record):
            with pytest.raises(B.BdrError) as e:
                call([rings[0], wrong])
            assert "member 1" in str(e.value) and word in str(e.value), (word, str(e.value))
    # profiling switched on for a member after the group was created
    g.members[1].profile_enable(True)
    for call in (g.opt, g.opt_with_record):
        with pytest.raises(B.BdrError) as e:
            call(rings)
        assert "member 1" in str(e.value) and "profiling" in str(e.value), str(e.value)
    g.members[1].profile_enable(False)
    with pytest.raises(ValueError):
        g.opt([rings[0]])
    with pytest.raises(B.BdrError, match="group"):
        g.members[0].close()
    assert g.kernel_launches == 0 and [m.n_opts for m in g.members] == [0, 0]
    for _ in range(2): g.opt(rings)
    g.sync()
    # counters, stream positions and parameters are those of two opts from a fresh start
    for i in range(2):
        assert_same(state(g.members[i], rings[i], shape), stepped_alone(B, shape, i, 2), i)
    g.close()
    for r in rings + [per, empty, other, xoshiro, store]: r.close()


# the smallest shape the host path of a round needs: obs 4, act 2, one hidden layer of 64, B = 33 (two row blocks, the last partial)
TINY = (4, 2, (64,), (64,), (64,), "None", 2, 33, ("Clamp", "Mse", False))


def test_a_buffer_closed_since_the_last_opt_and_a_null_buffer_are_refused_and_move_nothing(B):
    """opt() without buffers steps on the buffers named last: one closed since is refused here, naming the member, before the library
    sees its stale handle; a None buffer is the library's own refusal, not an AttributeError"""
    g = B.IqlGroup.build([config(B, TINY, i) for i in range(2)])
    rings = [ring(B, TINY, 100 + i) for i in range(2)]
    g.opt(rings)
    g.sync()
    trained, targets = models(TINY)
    moved = lambda: [{**{(m, r): a.get_params(m, role=r) for m in trained for r in ROLES}, **{(m, "param"): a.get_params(m) for m in targets}} for a in g.members]
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
