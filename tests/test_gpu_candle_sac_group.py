"""CandleSacGroup (csrc/candle_sac_group.hpp through the C ABI) against its twins: the same configs built as standalone CandleSac agents,
stepped one after the other on rings holding the same rows with the same seeds.  Everything is compared bit for bit (np.array_equal): a
group round runs the bodies of the standalone kernels on the same arguments, and draws its noise where the standalone update draws it.

Rings have capacity 128 and hold 100 random rows, `term` at rate 0.1.  The shapes are the smallest at which a kernel can still go wrong:
  name           obs act  critic / actor units          actor NC  B   limit, loss       what it reaches
  partial_block  17  6    (64,48) / (64,48)             Mlp2  2   7   Clamp, Mse        G = 8, one partial workgroup of rows, padded widths, the 2 A-wide
                                                                                        last layer, the z = 4 forward
  pen            45  24   (256,256) both                Mlp2  2   41  Tanh, SmoothL1    G = 32 with a partial last workgroup (8 rows each), two dense row
                                                                                        blocks, 25 actor-grad workgroups
  no_hidden      9   4    () / (64,), critic ReLU out   Mlp3  1   33  Clamp, Mse        dq/da is the unmasked input layer alone, no critic dX in the step,
                                                                                        the relu_out masks of qmin and critic loss, head2 and gh2
  wide_action    21  70   (64,64,64) / (128,)           Mlp3  2   20  Clamp, Mse        G = 64 with two columns per lane, unequal depth, 71 actor-grad
                                                                                        workgroups
  one_action     3   1    (64,64) both                  Mlp2  2   34  Tanh scale 2, Mse G = 1, the pendulum shape
11 rounds (more than the staging depth of 8, so slots are rewritten), round 5 an opt_with_record, and after round 6 one member takes
an update_on_batch of its own (member 1; member 0 in a group of one), as does its twin.  Member i differs from member 0 in seed,
gamma, critic_tau, the action limit's bounds / scale, the log-std clamps, both learning rates, Adam (even) against AdamW with weight
decay (odd), and the entropy mode: even members Auto with their own target entropy and learning rate, odd members Fix.
Scenarios: "train" / "eval" (all members), "mixmode" (even members train, odd members eval), "toggle" (the own member goes to eval mode
between rounds 3 and 4 and back to train mode after round 7), "interleave" (the own member calls its own train-mode sample after round
2, and the whole group acts through CandleSacGroup.sample after round 4 and after round 9: rounds, group acting and the member's own
calls continue ONE counter stream; the twin makes the same calls standalone), "online" (every member's ring takes 7 new rows through
rb.push after every round: it grows to its capacity after round 4 and wraps from then on).  state() ends with eight draws of the
member's noise stream, so a counter that is off by one draw shows even where no later round would.
A twin depends on its index, the scenario and on whether it is the own member, not on P: each is computed once and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# obs, act, critic units, actor units, critic activation_out, NC, B, (action limit, critic loss), actor kind, Tanh base scale
SHAPES = {
    "partial_block": (17, 6, (64, 48), (64, 48), "None", 2, 7, ("Clamp", "Mse"), "Mlp2", 1.0),
    "pen": (45, 24, (256, 256), (256, 256), "None", 2, 41, ("Tanh", "SmoothL1"), "Mlp2", 1.0),
    "no_hidden": (9, 4, (), (64,), "ReLU", 1, 33, ("Clamp", "Mse"), "Mlp3", 1.0),
    "wide_action": (21, 70, (64, 64, 64), (128,), "None", 2, 20, ("Clamp", "Mse"), "Mlp3", 1.0),
    "one_action": (3, 1, (64, 64), (64, 64), "None", 2, 34, ("Tanh", "Mse"), "Mlp2", 2.0),
}
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
PROBES = ("a", "logp", "q_min", "next_a", "next_logp", "tgt", "q_pred", "dq_da")
KEYS = ("loss_critic", "loss_actor", "ent_coef")
ROUNDS, RECORD_ROUND, OWN_UPDATE_AFTER = 11, 5, 6
TOGGLE_OFF_AFTER, TOGGLE_ON_AFTER = 3, 7
OWN_SAMPLE_AFTER, GROUP_SAMPLE_AFTER = 2, (4, 9)
N_ROWS, PUSH_ROWS = 100, 7


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
    Lq, Lp = len(shape[2]) + 1, len(shape[3]) + 1
    return 3 * Lp + 4 * Lq + 10


def in_train(scen, i):
    return {"eval": False, "mixmode": i % 2 == 0}.get(scen, True)


def config(B, shape, i, mixed=False, train=True, **kw):
    """member i: everything the group leaves free differs from member 0's; mixed: critic_loss and the action limit vary too"""
    od, ad, qu, pu, act_out, nc, bsz, (limit, closs), kind, scale = shape
    if mixed:
        limit, closs = ("Clamp", "Tanh", "Clamp")[i % 3], ("Mse", "SmoothL1")[i % 2]

    def opt(lr):
        return B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
    from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, MultiCriticConfig
    lim = ActionLimit.Tanh(scale + 0.25 * i) if limit == "Tanh" else ActionLimit.Clamp(-1.0 + 0.1 * i, 1.0 - 0.05 * i)
    ent = B.EntCoefMode.Auto(-0.5 * ad * (1 + 0.1 * i), 3e-3 * (1 + i)) if i % 2 == 0 else B.EntCoefMode.Fix(0.2 + 0.1 * i)
    c = B.CandleSacConfig(obs_dim=od, act_dim=ad,
                          critic_config=MultiCriticConfig(nc, CandleMlpConfig(tuple(qu), act_out), opt(2e-3 * (1 + 0.25 * i)), 0.005 * (1 + i)),
                          actor_config=GaussianActorConfig(CandleMlpConfig(tuple(pu), "None"), opt(5e-4 * (1 + i)), min_log_std=-5.0 - i,
                                                           max_log_std=2.0 - 0.5 * i, action_limit=lim, kind=kind),
                          gamma=0.99 - 0.02 * i, ent_coef_mode=ent, batch_size=bsz, critic_loss=closs, train=train, seed=3 + i, device=0)
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
    return rows(shape, 5000 + i, shape[6])


def pushed_rows(shape, i, k):
    """the rows member i's ring takes after round k of the online scenario"""
    return rows(shape, 9000 + 100 * i + k, PUSH_ROWS)


def act_rows(shape, i, k):
    """the observation rows member i acts on after round k (3 rows)"""
    return np.random.default_rng(7000 + 10 * i + k).standard_normal((3, shape[0])).astype(np.float32)


def models(shape):
    nc = shape[5]
    return ["actor"] + [f"critic_{i}" for i in range(nc)] + ["log_alpha"], [f"critic_tgt_{i}" for i in range(nc)]


def state(a, rb, shape):
    bsz = shape[6]
    trained, targets = models(shape)
    out = {(m, r): a.get_params(m, role=r) for m in trained for r in ROLES}
    out.update({(m, "param"): a.get_params(m) for m in targets})
    out.update({("probe", p): a.probe(p, bsz) for p in PROBES})
    out["n_opts"] = a.n_opts
    out["next_ixs"] = rb.sample_indices(8)
    out["next_noise"] = a.draw_noise(8)   # (last: it moves the counter)
    return out


def assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (tag, k)


def rec_bits(rec):
    return [np.float32(rec[k]).view(np.uint32) for k in KEYS]


@functools.lru_cache(maxsize=None)
def twin(name, i, own, mixed=False, scen="train"):
    """member i's twin, stepped alone: (state, the record of round 5, the actions of its acting calls)"""
    B, shape = lib(), SHAPES[name]
    a, rb = B.CandleSac.build(config(B, shape, i, mixed, in_train(scen, i))), ring(B, shape, 100 + i)
    rec, acts = None, []
    for k in range(1, ROUNDS + 1):
        if k == RECORD_ROUND: rec = a.opt_with_record(rb)
        else: a.opt(rb)
        if k == OWN_UPDATE_AFTER and own: a.update_on_batch(*own_batch(shape, i))
        if scen == "toggle" and own:
            if k == TOGGLE_OFF_AFTER: a.eval()
            if k == TOGGLE_ON_AFTER: a.train()
        if scen == "interleave":
            if k == OWN_SAMPLE_AFTER and own: acts.append(a.sample(act_rows(shape, i, k)))
            if k in GROUP_SAMPLE_AFTER: acts.append(a.sample_raw(act_rows(shape, i, k)))
        if scen == "online": rb.push(*pushed_rows(shape, i, k))
    a.sync()
    out = (state(a, rb, shape), rec, acts)
    a.close(); rb.close()
    return out


def run_group(B, name, P, mixed=False, scen="train"):
    shape = SHAPES[name]
    own = min(1, P - 1)
    g = B.CandleSacGroup.build([config(B, shape, i, mixed, in_train(scen, i)) for i in range(P)])
    rings = [ring(B, shape, 100 + i) for i in range(P)]
    count = launch_count(shape)
    assert len(g) == P and g.form == "candle_sac_layers" and g.launches_per_round == count and g.kernel_launches == 0
    recs, acts, n_act = None, [[] for _ in range(P)], 0
    for k in range(1, ROUNDS + 1):
        if k == RECORD_ROUND: recs = g.opt_with_record()
        else: g.opt(rings if k == 1 else None)
        if k == OWN_UPDATE_AFTER: g.members[own].update_on_batch(*own_batch(shape, own))
        if scen == "toggle":
            if k == TOGGLE_OFF_AFTER: g.members[own].eval()
            if k == TOGGLE_ON_AFTER: g.members[own].train()
        if scen == "interleave":
            if k == OWN_SAMPLE_AFTER: acts[own].append(g.members[own].sample(act_rows(shape, own, k)))
            if k in GROUP_SAMPLE_AFTER:
                for i, a in enumerate(g.sample([act_rows(shape, i, k) for i in range(P)])): acts[i].append(a)
                n_act += 1
        if scen == "online":
            for i, rb in enumerate(rings): rb.push(*pushed_rows(shape, i, k))
    g.sync()
    assert g.kernel_launches == ROUNDS * count + n_act          # rounds x count, and one launch per group acting call
    for i, (m, rb) in enumerate(zip(g.members, rings)):
        want, want_rec, want_acts = twin(name, i, i == own, mixed, scen)
        assert_same(state(m, rb, shape), want, (name, P, i, scen))
        assert list(recs[i]) == list(KEYS) and rec_bits(recs[i]) == rec_bits(want_rec), (name, P, i, recs[i], want_rec)
        assert m.n_opts == ROUNDS + (1 if i == own else 0)
        assert len(acts[i]) == len(want_acts) and all(np.array_equal(x, y) for x, y in zip(acts[i], want_acts)), (name, P, i, "actions")
    g.close()
    for rb in rings: rb.close()


@pytest.mark.parametrize("scen", ["train", "eval"])
@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_group_equals_its_twins_bit_for_bit(B, name, P, scen):
    run_group(B, name, P, scen=scen)


def test_the_launch_count_is_the_formula(B):
    for name, want in (("partial_block", 31), ("pen", 31), ("no_hidden", 20), ("wide_action", 32), ("one_action", 31)):
        assert launch_count(SHAPES[name]) == want
    # (run_group compares launches_per_round with it for every shape, and kernel_launches with rounds x count + the acting calls)


def test_members_of_one_group_may_be_in_different_modes(B):
    run_group(B, "partial_block", 5, scen="mixmode")


def test_set_train_on_a_member_between_rounds_takes_effect_in_the_next_round(B):
    run_group(B, "partial_block", 2, scen="toggle")
    run_group(B, "pen", 5, scen="toggle")


def test_rounds_group_acting_and_a_members_own_sample_continue_one_noise_stream(B):
    run_group(B, "partial_block", 2, scen="interleave")
    run_group(B, "wide_action", 5, scen="interleave")


def test_online_members_whose_rings_grow_and_wrap_between_rounds(B):
    assert N_ROWS + 4 * PUSH_ROWS == 128 and N_ROWS + ROUNDS * PUSH_ROWS > 128   # full after round 4, wrapped by the end
    run_group(B, "partial_block", 2, scen="online")
    run_group(B, "one_action", 5, scen="online")


def test_members_may_mix_critic_loss_action_limit_and_entropy_mode(B):
    cfgs = [config(B, SHAPES["partial_block"], i, True) for i in range(5)]
    assert len({c.critic_loss for c in cfgs}) == 2 and len({c.actor_config.action_limit.kind for c in cfgs}) == 2
    assert len({c.ent_coef_mode.kind for c in cfgs}) == 2
    run_group(B, "partial_block", 5, mixed=True)


def test_a_group_over_views_of_one_ring_equals_its_twins_on_three_rings(B):
    shape = SHAPES["partial_block"]
    data = rows(shape, 21)
    owner = ring(B, shape, 99, data)
    views = [owner.view(50 + i) for i in range(3)]
    g = B.CandleSacGroup.build([config(B, shape, i) for i in range(3)])
    g.opt(views)
    recs = g.opt_with_record()
    g.opt()
    g.sync()
    for i in range(3):
        a, rb = B.CandleSac.build(config(B, shape, i)), ring(B, shape, 50 + i, data)
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
    a, rb = B.CandleSac.build(config(B, shape, i)), ring(B, shape, 100 + i)
    for _ in range(n): a.opt(rb)
    a.sync()
    out = state(a, rb, shape)
    a.close(); rb.close()
    return out


@pytest.mark.parametrize("what", ["second_shape", "actor_kind", "three_critics", "two_updates", "not_candle_sac", "twice"])
def test_a_member_that_cannot_join_is_named_and_nobody_is_adopted(B, what):
    shape = SHAPES["partial_block"]
    first = B.CandleSac.build(config(B, shape, 0))
    if what == "second_shape":
        bad = B.CandleSac.build(config(B, SHAPES["one_action"], 1, batch_size=shape[6]))
    elif what == "actor_kind":
        c = config(B, shape, 1)
        c.actor_config.kind = "Mlp3"
        bad = B.CandleSac.build(c)
    elif what == "three_critics":
        c = config(B, shape, 1)
        c.critic_config.n_nets = 3
        bad = B.CandleSac.build(c)
    elif what == "two_updates":
        bad = B.CandleSac.build(config(B, shape, 1, n_updates_per_opt=2))
    elif what == "not_candle_sac":
        from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, MultiCriticConfig
        bad = B.Awac.build(B.AwacConfig(obs_dim=shape[0], act_dim=shape[1], critic_config=MultiCriticConfig(2, CandleMlpConfig((64, 48), "None")),
                                        actor_config=GaussianActorConfig(CandleMlpConfig((64, 48), "None")), batch_size=shape[6], device=0, seed=1))
    else:
        bad = first
    with pytest.raises(B.BdrError, match="member 1"):
        B.CandleSacGroup([first, bad])
    # nothing moved: member 0 is still a standalone agent and steps as its twin does
    rb = ring(B, shape, 100)
    for _ in range(2): first.opt(rb)
    first.sync()
    assert_same(state(first, rb, shape), stepped_alone(B, shape, 0, 2), what)
    first.close(); rb.close()
    if bad is not first: bad.close()


# observation rows of 16 bytes: the width a single-frame store of one frame can have
STORE_SHAPE = (4, 6, (64, 48), (64, 48), "None", 2, 7, ("Clamp", "Mse"), "Mlp2", 1.0)


def test_refused_buffers_name_the_member_and_move_nothing(B):
    """every buffer rule of a grouped opt, with member 1 the one concerned: member 0 has a good ring, so a check made only once the
    round is under way would have moved member 0's step counters, n_opts, noise counter (the members are in train mode) and stream
    position before it refused"""
    shape = STORE_SHAPE
    cfg = lambda **kw: B.SimpleReplayBufferConfig(capacity=128, **kw)
    g = B.CandleSacGroup.build([config(B, shape, i) for i in range(2)])
    assert all(m.is_train() for m in g.members)
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
    # the three step counters, noise counters, stream positions and parameters are those of two opts from a fresh start
    for i in range(2):
        assert_same(state(g.members[i], rings[i], shape), stepped_alone(B, shape, i, 2), i)
    g.close()
    for r in rings + [per, empty, other, xoshiro, store]: r.close()


def test_a_record_needs_room_for_three_values(B):
    import ctypes as C
    from border_amd import _lib
    shape = SHAPES["partial_block"]
    g = B.CandleSacGroup.build([config(B, shape, 0)])
    rb = ring(B, shape, 100)
    out, cnt = np.zeros(2, np.float32), np.zeros(1, np.int32)
    hs = (C.c_void_p * 1)(rb.handle)
    st = _lib.lib().bdr_candle_sac_group_opt_with_scalars(g.handle, hs, out.ctypes.data_as(C.c_void_p), 2, cnt.ctypes.data_as(C.c_void_p))
    assert st != 0 and b"three keys" in _lib.lib().bdr_last_error()
    assert g.kernel_launches == 0 and g.members[0].n_opts == 0
    g.close(); rb.close()
