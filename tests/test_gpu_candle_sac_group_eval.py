"""CandleSacGroup.evaluate (bdr_evaluate_bc_group behind the candle SAC's table, over k_candle_act_group) against Evaluator.evaluate
member after member, and CandleSacGroup.train_offline with post-processing (bdr_trainer_train_offline_group_post) against standalone
CandleSac twins run through bdr_trainer_train_offline_post on rings of the same rows and seeds.  The members have Mlp2 actors; even
members tune their entropy coefficient (Auto), odd members keep it (Fix).  The offline loop puts the members in train mode for its
update rounds, so every round draws a and next_a from the member's noise stream, and in eval mode for the evaluations in between.
Everything is compared bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (17, 6, (64, 48), 7)   # obs, act, actor units, batch: padded widths, one partial row block; the critic is (64,)
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
TRAINED, TARGETS = ("actor", "critic_0", "critic_1", "log_alpha"), ("critic_tgt_0", "critic_tgt_1")
KEYS = ("loss_critic", "loss_actor", "ent_coef")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def config(B, i):
    from border_amd.iql import ActionLimit, CandleMlpConfig, GaussianActorConfig, MultiCriticConfig
    od, ad, un, bsz = SHAPE
    lr = 1e-3 * (1 + 0.5 * i)
    opt = lambda: B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
    limit = ActionLimit.Tanh(1.0 + 0.25 * i) if i % 2 else ActionLimit.Clamp(-0.5 - 0.1 * i, 0.6 + 0.1 * i)
    ent = B.EntCoefMode.Auto(-0.5 * ad, 3e-3 * (1 + i)) if i % 2 == 0 else B.EntCoefMode.Fix(0.2 + 0.1 * i)
    return B.CandleSacConfig(obs_dim=od, act_dim=ad, critic_config=MultiCriticConfig(2, CandleMlpConfig((64,)), opt(), 0.005 * (1 + i)),
                             actor_config=GaussianActorConfig(CandleMlpConfig(tuple(un)), opt(), min_log_std=-3.0 + 0.5 * i, max_log_std=1.0 - 0.2 * i,
                                                              action_limit=limit, kind="Mlp2"),
                             ent_coef_mode=ent, gamma=0.99 - 0.02 * i, batch_size=bsz, seed=3 + i, device=0)


def ring(B, seed):
    od, ad = SHAPE[0], SHAPE[1]
    rng = np.random.default_rng(1000 + seed)
    n = 100
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=128, seed=seed), (od,), np.float32, (ad,), np.float32, device=0)
    rb.push(rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32),
            rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.1).astype(np.int8),
            np.zeros(n, np.int8))
    return rb


class ScriptedEnv:
    """Member m's evaluation environment: episode ix has lengths[ix] steps (the last one terminates, or truncates for odd ix), the
    observation is a fixed function of (m, ix, t) and the reward the f32 sum of the action row, so the score carries the action bits.
    Every action row is logged as bytes."""
    def __init__(self, m, lengths):
        self.m, self.lengths, self.actions, self.ix, self.t = m, lengths, [], 0, 0

    def obs(self):
        return 2.0 * np.sin(0.37 * np.arange(SHAPE[0], dtype=np.float64) + self.m + 3.0 * self.ix + 0.5 * self.t)

    def reset_with_index(self, ix):
        self.ix, self.t = ix, 0
        return self.obs()

    def step(self, act):
        self.actions.append((self.ix, self.t, act.tobytes()))
        self.t += 1
        done = self.t == self.lengths[self.ix]
        return self.obs(), float(np.sum(act, dtype=np.float32)), done and self.ix % 2 == 0, done and self.ix % 2 == 1


def normaliser(B):
    rng = np.random.default_rng(900)
    return B.ObsNormalizer(SHAPE[0], 0).set(rng.standard_normal(SHAPE[0]).astype(np.float32), rng.uniform(0.5, 2.0, SHAPE[0]).astype(np.float32))


# per member: episode lengths (their count = n_episodes), the rows' dtype, a normaliser or not, reference scores or not
PLANS = [([3, 1], np.float64, True, None), ([2, 2, 4], np.float32, False, (-1.5, 9.25)), ([5], np.float64, False, None)]


def evaluators(B, nz, plans=PLANS):
    return [B.Evaluator(ScriptedEnv(m, lengths), len(lengths), obs_norm=nz if with_norm else None, obs_dtype=dtype, ref_scores=refs, obs_dim=SHAPE[0],
                        act_dim=SHAPE[1], act_dtype=np.float32) for m, (lengths, dtype, with_norm, refs) in enumerate(plans)]


def f32_bits(x):
    return None if x is None else np.float32(x).tobytes()


def same_result(got, want):
    return (f32_bits(got.score), f32_bits(got.normalized), got.n_steps, got.n_episodes) == \
           (f32_bits(want.score), f32_bits(want.normalized), want.n_steps, want.n_episodes)


def test_eval_mode_group_evaluate_equals_evaluator_evaluate_member_after_member(B):
    P = len(PLANS)
    g = B.CandleSacGroup.build([config(B, i) for i in range(P)])
    nz = normaliser(B)
    evs = evaluators(B, nz)
    before = g.kernel_launches
    got = g.evaluate(evs)
    rounds = max(sum(p[0]) for p in PLANS)
    assert g.kernel_launches == before + rounds          # ONE acting launch per round, over the members with an open episode
    for m, member in enumerate(g.members):
        alone = evaluators(B, nz)[m]
        want = alone.evaluate(member)
        assert same_result(got[m], want), m
        assert evs[m].env.actions == alone.env.actions and len(alone.env.actions) == sum(PLANS[m][0]), m
        assert member.n_opts == 0
    assert got[1].normalized is not None and got[0].normalized is None
    g.close(); nz.close()


def test_train_mode_group_evaluate_equals_the_twins_and_finished_members_take_no_draws(B):
    P = len(PLANS)
    g, tw = B.CandleSacGroup.build([config(B, i) for i in range(P)]), [B.CandleSac.build(config(B, i)) for i in range(P)]
    for a in g.members + tw: a.train()
    nz = normaliser(B)
    evs = evaluators(B, nz)
    got = g.evaluate(evs)
    for m in range(P):
        alone = evaluators(B, nz)[m]
        want = alone.evaluate(tw[m])
        assert same_result(got[m], want), m
        assert evs[m].env.actions == alone.env.actions and len(alone.env.actions) == sum(PLANS[m][0]), m
        # a member that finished early left the selection: its stream stands where its twin's stands, n_steps * A draws on
        assert np.array_equal(g.members[m].draw_noise(7), tw[m].draw_noise(7)), m
    g.close(); nz.close()
    for t in tw: t.close()


def test_an_evaluator_whose_action_row_is_not_the_members_is_refused(B):
    g = B.CandleSacGroup.build([config(B, i) for i in range(2)])
    evs = [B.Evaluator(ScriptedEnv(m, [1]), 1, obs_dim=SHAPE[0], act_dim=SHAPE[1] + (m == 1), act_dtype=np.float32) for m in range(2)]
    with pytest.raises(B.BdrError, match="member 1: a candle SAC group"):
        g.evaluate(evs)
    assert g.kernel_launches == 0 and evs[0].env.actions == []
    g.close()


def files_under(root):
    out = {}
    for d, _, names in os.walk(root):
        for f in names:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def models_of(a):
    out = {(m, r): a.get_params(m, role=r) for m in TRAINED for r in ROLES}
    out.update({(m, "param"): a.get_params(m) for m in TARGETS})
    return out


P_TRAIN, MAX_OPTS, RECORD = 2, 6, 4


@pytest.fixture(scope="module")
def twin_runs(B, tmp_path_factory):
    """the twins, once: bdr_trainer_train_offline_post of a lone agent"""
    root = tmp_path_factory.mktemp("candle_sac_twins")
    nz = normaliser(B)
    want = []
    for i in range(P_TRAIN):
        a, rb, ev, events = B.CandleSac.build(config(B, i)), ring(B, 100 + i), evaluators(B, nz, PLANS[:P_TRAIN])[i], []
        B.NativeTrainer(B.TrainerConfig(max_opts=MAX_OPTS, record_agent_info_interval=RECORD)).train_offline(
            a, rb, on_event=lambda *e: events.append(e), evaluator=ev, eval_interval=2, save_interval=3, model_dir=str(root / f"twin{i}"))
        a.sync()
        want.append((models_of(a), a.n_opts, events, ev.env.actions, files_under(root / f"twin{i}")))
        a.close(); rb.close()
    nz.close()
    return want


def raw_train_offline_null_save(B, g, rings, evs, dirs, on_event):
    """bdr_trainer_train_offline_group_post as a C caller that leaves save_member NULL: the fallback is chosen by the evaluation table"""
    from border_amd import _lib
    from border_amd.trainer import NativeTrainer
    n = len(g)
    ops, post, c = _lib.GroupTrainerOps(), _lib.BcGroupTrainerPostC(), _lib.TrainerConfigC()
    bufs = (C.c_void_p * n)(*[b.handle for b in rings])
    _lib.lib().bdr_candle_sac_group_trainer_ops_default(C.byref(ops), g.handle, bufs)
    _lib.lib().bdr_candle_sac_group_trainer_post_default(C.byref(post), g.handle)
    post.save_member = _lib.G_SAVE_MEMBER_FN()                                # NULL
    assert not post.save_member
    _lib.lib().bdr_trainer_config_default(C.byref(c))
    c.max_opts, c.record_agent_info_interval = MAX_OPTS, RECORD
    post.eval_interval, post.save_interval = 2, 3
    cev = (_lib.EvaluatorC * n)(*[e.c_struct() for e in evs])
    post.evaluators = cev
    cdirs = (C.c_char_p * n)(*[str(d).encode() for d in dirs])
    post.model_dirs = cdirs
    cb = _lib.GROUP_OBSERVER_FN(lambda _c, m, es, os_, ev, sc, k: on_event(m, es, os_, NativeTrainer.EVENTS[ev], [sc[i] for i in range(k)]))
    st = (_lib.TrainerStatsC * n)()
    _lib.check(_lib.lib().bdr_trainer_train_offline_group_post(C.byref(c), C.byref(ops), C.byref(post), cb, None, st))
    g.sync()


@pytest.mark.parametrize("null_save", [False, True])
def test_train_offline_with_post_processing_equals_the_standalone_twins(B, twin_runs, null_save, tmp_path):
    P, plans = P_TRAIN, PLANS[:P_TRAIN]
    nz = normaliser(B)
    g = B.CandleSacGroup.build([config(B, i) for i in range(P)])
    rings, evs, events, records = [ring(B, 100 + i) for i in range(P)], evaluators(B, nz, plans), [], []
    dirs = [str(tmp_path / f"group{i}") for i in range(P)]
    if null_save:
        raw_train_offline_null_save(B, g, rings, evs, dirs, lambda *e: events.append(e))
    else:
        stats = g.train_offline(rings, MAX_OPTS, record_interval=RECORD, on_record=lambda k, r: records.append((k, r)), evaluators=evs, eval_interval=2,
                                save_interval=3, model_dirs=dirs, on_event=lambda *e: events.append(e))
        assert [k for k, _ in records] == [4] and all(s["opt_steps"] == MAX_OPTS and s["n_records"] == 1 for s in stats)
        assert all(tuple(r.keys()) == KEYS for r in records[0][1])
    n_eval_launches = 3 * max(sum(p[0]) for p in plans)
    assert g.kernel_launches == MAX_OPTS * g.launches_per_round + n_eval_launches
    for i, m in enumerate(g.members):
        models, n_opts, ev_twin, actions, files = twin_runs[i]
        got = models_of(m)
        assert got.keys() == models.keys()
        for k in models:
            assert np.array_equal(got[k], models[k]), (i, k)
        assert m.n_opts == n_opts == MAX_OPTS
        mine = [e[1:] for e in events if e[0] == i]
        assert [(e, o, n, [np.float32(x).tobytes() for x in sc]) for e, o, n, sc in mine] == \
               [(e, o, n, [np.float32(x).tobytes() for x in sc]) for e, o, n, sc in ev_twin], i
        assert [n for _, _, n, _ in mine] == ["opt", "opt", "eval", "opt", "opt_record", "eval", "opt", "opt", "eval"]
        if not null_save:
            assert [np.float32(records[0][1][i][k]) for k in KEYS] == [np.float32(x) for x in ev_twin[4][3]]
        assert evs[i].env.actions == actions
        got_files = files_under(tmp_path / f"group{i}")
        assert got_files == files and {os.path.dirname(k) for k in files} == {"best", "3", "6"}, (i, sorted(got_files))
    g.close(); nz.close()
    for rb in rings: rb.close()
