"""CandleDqnGroup (csrc/candle_dqn_group.hpp through the C ABI) against its twins: the same configs built as standalone CandleDqn agents,
stepped one after the other on rings holding the same rows with the same seeds.  Everything is compared with == on the raw bits: a
group round runs the bodies of the standalone kernels on the same arguments.

Rings have capacity 128 and hold 100 random rows, `term` at rate 0.1.  The shapes are the smallest at which a kernel can still go wrong:
  name            obs  A   units       B   double  out   what it reaches
  cartpole_small  4    2   (64, 64)    64  no      None  two row blocks, L = 3 (10 launches), the z = 2 forward
  odd_double      70   33  (128,)      37  yes     None  a partial row block, Kp = 128 > obs, padded action columns, the z = 3 forward
  no_hidden       9    5   ()          33  no      None  L = 1: no input gradient, the TD launch's dy feeds the weight gradient directly
  seven_layers    6    3   (64,) * 6   16  yes     None  L = 7: six input gradients, seven reduce segments
  relu_out        4    2   (64, 64)    64  no      ReLU  the closed-ReLU branch of the TD launch's gradient rows
Three rounds, the last one an opt_with_record.  Member i differs from member 0 in seed, learning rate, Adam (even) against AdamW with
weight decay (odd), discount, tau, soft_update_interval (1, 2, 3: rounds with and without a tracking member mix), Mse (even) against
smooth-l1 (odd) and record verbosity (0, 2, 0, ...).  A twin depends on its index and the shape, not on P: each is computed once."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# obs, actions, units, batch, double_dqn, activation_out
SHAPES = {
    "cartpole_small": (4, 2, (64, 64), 64, False, "None"),
    "odd_double": (70, 33, (128,), 37, True, "None"),
    "no_hidden": (9, 5, (), 33, False, "None"),
    "seven_layers": (6, 3, (64,) * 6, 16, True, "None"),
    "relu_out": (4, 2, (64, 64), 64, False, "ReLU"),
}
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
PROBES = ("pred", "q_next", "y", "tgt", "dpred")
ROUNDS, N_ROWS = 3, 100


def lib():
    import border_amd
    return border_amd


@pytest.fixture(scope="module")
def B():
    border_amd = lib()
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def config(B, shape, i, train=False, explorer=None, **kw):
    """member i: everything the group leaves free differs from member 0's"""
    od, A, units, bsz, dd, act_out = shape
    from border_amd.iql import CandleMlpConfig
    lr = 1e-3 * (1 + 0.5 * i)
    opt = B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
    c = B.CandleDqnConfig(obs_dim=od, n_actions=A, model_config=B.CandleDqnModelConfig(CandleMlpConfig(tuple(units), act_out), opt),
                          soft_update_interval=1 + i % 3, batch_size=bsz, discount_factor=0.99 - 0.03 * i, tau=0.005 * (1 + i), train=train,
                          explorer=explorer if explorer is not None else B.Softmax(), explorer_seed=42 + i, double_dqn=dd,
                          critic_loss=("Mse", "SmoothL1")[i % 2], record_verbose_level=(0, 2)[i % 2], seed=3 + i, device=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def rows(shape, seed, n=N_ROWS):
    od, A = shape[0], shape[1]
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, od)).astype(np.float32), rng.integers(0, A, (n, 1)).astype(np.int64), rng.standard_normal((n, od)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.1).astype(np.int8), np.zeros(n, np.int8))


def ring(B, shape, seed, data=None, per=False, fill=True, capacity=128):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed, per_config=B.PerConfig() if per else None),
                              (shape[0],), np.float32, (1,), np.int64, device=0)
    if fill:
        rb.push(*(data if data is not None else rows(shape, 1000 + seed)))
    return rb


def state(a, rb, shape):
    bsz = shape[3]
    out = {("qnet", r): a.get_params("qnet", r) for r in ROLES}
    out[("qnet_tgt", "param")] = a.get_params("qnet_tgt")
    out.update({("probe", p): a.probe(p, bsz) for p in PROBES})
    out["n_opts"] = a.n_opts
    out["next_ixs"] = rb.sample_indices(8)
    return out


def assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        assert (bits(got[k]) == bits(want[k])).all(), (tag, k)


def rec_bits(rec):
    return [(k, np.float32(v).view(np.uint32)) for k, v in rec.items()]


@functools.lru_cache(maxsize=None)
def twin(name, i, shared_rows=False, train=False):
    """member i's twin, stepped alone: (state, the record of the last round).  shared_rows: its ring holds member 0's rows (what a view
    of one ring reads) with its own index stream"""
    B, shape = lib(), SHAPES[name]
    a = B.CandleDqn.build(config(B, shape, i, train=train))
    rb = ring(B, shape, 100 + i, data=rows(shape, 1100) if shared_rows else None)
    rec = None
    for k in range(1, ROUNDS + 1):
        if k == ROUNDS: rec = a.opt_with_record(rb)
        else: a.opt(rb)
    a.sync()
    out = (state(a, rb, shape), rec)
    a.close(); rb.close()
    return out


def run_group(B, name, P, views=False, train=None):
    shape = SHAPES[name]
    train = train or (lambda i: False)
    g = B.CandleDqnGroup.build([config(B, shape, i, train=train(i)) for i in range(P)])
    owner = None
    if views:
        owner = ring(B, shape, 999, data=rows(shape, 1100))
        bufs = [owner.view(100 + i) for i in range(P)]
    else:
        bufs = [ring(B, shape, 100 + i) for i in range(P)]
    base = g.kernel_launches
    recs = None
    for k in range(1, ROUNDS + 1):
        if k == ROUNDS: recs = g.opt_with_record(bufs)
        else: g.opt(bufs)
    launches = g.kernel_launches - base
    g.sync()
    states = [state(g.members[i], bufs[i], shape) for i in range(P)]
    info = g.info()
    g.close()
    for rb in bufs: rb.close()
    if owner is not None: owner.close()
    return states, recs, launches, info


@pytest.mark.parametrize("views", [False, True], ids=["rings", "views"])
@pytest.mark.parametrize("P", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rounds_equal_the_members_stepped_alone(B, name, P, views):
    states, recs, launches, info = run_group(B, name, P, views)
    L = len(SHAPES[name][2]) + 1
    assert info["form"] == "candle_dqn_layers" and info["n_members"] == P and info["launches_per_round"] == 2 * L + 4
    assert launches == ROUNDS * (2 * L + 4)              # whatever P is
    for i in range(P):
        want, want_rec = twin(name, i, shared_rows=views)
        assert_same(states[i], want, (name, P, i))
        assert rec_bits(recs[i]) == rec_bits(want_rec), (name, P, i)
        assert list(recs[i])[0] == "loss" and list(recs[i])[-1] == "ratio_best_act"
        assert ("pred_mean" in recs[i]) == (i % 2 == 1)   # verbosity 2 on the odd members: the four means and the parameter statistics


def test_a_member_in_eval_mode_beside_members_in_train_mode(B):
    name = "cartpole_small"
    states, recs, _l, _i = run_group(B, name, 3, train=lambda i: i != 1)
    for i in range(3):
        want, want_rec = twin(name, i, train=(i != 1))
        assert_same(states[i], want, i)
        assert rec_bits(recs[i]) == rec_bits(want_rec), i


def test_a_member_with_an_out_of_range_action_is_skipped_reported_and_steps_again(B):
    """member 1's ring holds ONE row whose action is n_actions; capacity 8 and batch 64, so every batch draws it.  The kernel clamps the
    index (no out-of-bounds access); the member's reduce + Adam is skipped on the device, the others' is not."""
    name = "cartpole_small"
    shape = SHAPES[name]
    P, bad = 3, 1
    data = [rows(shape, 1000 + 100 + i, 8) for i in range(P)]
    poisoned = [d if i != bad else (d[0], np.concatenate([d[1][:5], [[shape[1]]], d[1][6:]]).astype(np.int64)) + d[2:] for i, d in enumerate(data)]
    g = B.CandleDqnGroup.build([config(B, shape, i) for i in range(P)])
    twins = [B.CandleDqn.build(config(B, shape, i)) for i in range(P)]
    bufs = [ring(B, shape, 100 + i, data=poisoned[i], capacity=8) for i in range(P)]
    tbufs = [ring(B, shape, 100 + i, data=poisoned[i], capacity=8) for i in range(P)]
    for _ in range(2):
        g.opt(bufs)
        for i in range(P): twins[i].opt(tbufs[i])
    with pytest.raises(B.BdrError, match=r"member 1: .*action index outside"):
        g.sync()
    for i in range(P):
        if i == bad:
            with pytest.raises(B.BdrError, match="action index outside"):
                twins[i].sync()
        else:
            twins[i].sync()
    g.sync()   # reported once: the word is cleared
    for i in range(P):
        assert g.members[i].n_opts == twins[i].n_opts == (0 if i == bad else 2), i
        assert_same(state(g.members[i], bufs[i], shape), state(twins[i], tbufs[i], shape), ("after the report", i))
    # the ring's row is overwritten (the ring wraps: 8 good rows replace all 8): the member steps again, with the step numbers and the
    # soft-update counter it would have had if the bad rounds had never been enqueued
    good = rows(shape, 4000, 8)
    bufs[bad].push(*good); tbufs[bad].push(*good)
    recs = None
    for _ in range(3):
        recs = g.opt_with_record(bufs)
        trecs = [twins[i].opt_with_record(tbufs[i]) for i in range(P)]
    for i in range(P):
        assert g.members[i].n_opts == twins[i].n_opts == (3 if i == bad else 5), i
        assert rec_bits(recs[i]) == rec_bits(trecs[i]), i
        assert_same(state(g.members[i], bufs[i], shape), state(twins[i], tbufs[i], shape), ("after the overwrite", i))
    g.close()
    for x in twins + bufs + tbufs: x.close()


def test_members_that_cannot_join_are_refused_and_nobody_is_adopted(B):
    from tests import test_gpu_candle_sac_group as TC
    shape = SHAPES["cartpole_small"]
    ok = lambda i: B.CandleDqn.build(config(B, shape, i))
    cases = {
        "shape": lambda: B.CandleDqn.build(config(B, shape, 1, batch_size=32)),
        "double_dqn": lambda: B.CandleDqn.build(config(B, shape, 1, double_dqn=True)),
        "n_updates_per_opt": lambda: B.CandleDqn.build(config(B, shape, 1, n_updates_per_opt=2)),
        "AtariCnn": lambda: B.CandleDqn.build(B.CandleDqnConfig(q_config=B.AtariCnnConfig(n_stack=1, out_dim=2), batch_size=2, device=0)),
        "not a candle DQN agent": lambda: B.CandleSac.build(TC.config(B, TC.SHAPES["one_action"], 0)),
    }
    for text, make in cases.items():
        other, a, b = make(), ok(0), ok(2)
        with pytest.raises(B.BdrError, match=r"member 1 cannot join a candle DQN group.*" + text):
            B.CandleDqnGroup([a, other, b])
        # nobody was adopted: every agent is still its own and steps alone
        rb = ring(B, shape, 7)
        a.opt(rb); b.opt(rb); a.sync(); b.sync()
        assert a.n_opts == b.n_opts == 1
        for x in (a, b, other, rb): x.close()
    a = ok(0)
    with pytest.raises(B.BdrError, match="member 1 cannot join a candle DQN group.*earlier member"):
        B.CandleDqnGroup([a, a])
    a.close()


def test_buffers_that_cannot_be_stepped_are_refused_before_anything_moves(B):
    shape = SHAPES["cartpole_small"]
    g = B.CandleDqnGroup.build([config(B, shape, i) for i in range(3)])
    twins = [B.CandleDqn.build(config(B, shape, i)) for i in range(3)]
    good, tb = [ring(B, shape, 100 + i) for i in range(3)], [ring(B, shape, 100 + i) for i in range(3)]
    g.opt(good); g.sync()
    for i in range(3):
        twins[i].opt(tb[i]); twins[i].sync()
    f32_act = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=128, seed=5), (shape[0],), np.float32, (1,), np.float32, device=0)
    d = rows(shape, 77)
    f32_act.push(d[0], d[1].astype(np.float32), *d[2:])
    cfg = lambda **kw: B.SimpleReplayBufferConfig(capacity=128, **kw)
    xoshiro = B.SimpleReplayBuffer(cfg(seed=10, index_rng="xoshiro256++"), (shape[0],), np.float32, (1,), np.int64, device=0)
    xoshiro.push(*rows(shape, 78))
    store = B.SimpleReplayBuffer(cfg(seed=11, frame_stack=1), (shape[0],), np.float32, (1,), np.int64, device=0)   # obs 4: 16-byte rows, one frame
    cases = {
        "prioritized": ring(B, shape, 9, per=True),
        "single-frame": store,                                     # a frame-stack store
        "StdRng": xoshiro,                                         # another index stream than the grouped gather draws
        "do not match": f32_act,                                   # 4-byte action rows
        "empty": ring(B, shape, 9, fill=False),
    }
    launches = g.kernel_launches
    for text, bad in cases.items():
        for call in (g.opt, g.opt_with_record):
            with pytest.raises(B.BdrError, match="member 1: .*" + text):
                call([good[0], bad, good[2]])
        bad.close()
    for call in (g.opt, g.opt_with_record):
        with pytest.raises(B.BdrError, match="member 2: .*shares its replay buffer"):
            call([good[0], good[1], good[0]])
        with pytest.raises(B.BdrError, match="member 0: null buffer"):
            call([None, good[1], good[2]])
    # (a ring on another device needs a second GPU: tests/test_candle_dqn_group_host.py covers the member's device, the buffer's is
    # one comparison in group_check_buffers)
    assert g.kernel_launches == launches
    g.sync()
    # nothing moved - no counter, no parameter, no index stream: the next round is the twins' second round
    for i in range(3):
        assert g.members[i].n_opts == 1
    g.opt(good); g.sync()
    for i in range(3):
        twins[i].opt(tb[i]); twins[i].sync()
        assert_same(state(g.members[i], good[i], shape), state(twins[i], tb[i], shape), i)
    g.close()
    for x in good + twins + tb: x.close()
