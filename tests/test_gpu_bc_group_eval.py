"""BcGroup.evaluate (bdr_evaluate_bc_group over k_bc_act_group) against Evaluator.evaluate member after member, and
BcGroup.train_offline with post-processing (bdr_trainer_train_offline_group_post) against standalone Bc twins run through
bdr_trainer_train_offline_post on rings of the same rows and seeds.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (17, 6, (64, 48), "None", 7)   # obs, act, units, activation_out, batch: padded widths, one partial row block
ROLES = ("param", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def config(B, i, form="general"):
    od, ad, un, act_out, bsz = SHAPE
    lr = 1e-3 * (1 + 0.5 * i)
    opt = B.OptimizerConfig.Adam(lr) if i % 2 == 0 else B.OptimizerConfig.AdamW(lr, 0.9, 0.999, 0.02, 1e-8)
    return B.BcConfig(obs_dim=od, act_dim=ad, policy_model_config=B.BcModelConfig(B.CandleMlpConfig(tuple(un), act_out), opt),
                      batch_size=bsz, action_type="Continuous", device=0, seed=3 + i, kernel_form=form)


def ring(B, seed):
    od, ad = SHAPE[0], SHAPE[1]
    rng = np.random.default_rng(1000 + seed)
    n = 100
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=128, seed=seed), (od,), np.float32, (ad,), np.float32, device=0)
    rb.push(rng.standard_normal((n, od)).astype(np.float32), rng.uniform(-0.9, 0.9, (n, ad)).astype(np.float32),
            rng.standard_normal((n, od)).astype(np.float32), rng.standard_normal(n).astype(np.float32), np.zeros(n, np.int8), np.zeros(n, np.int8))
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


def test_group_evaluate_equals_evaluator_evaluate_member_after_member(B):
    P = len(PLANS)
    g = B.BcGroup.build([config(B, i) for i in range(P)])
    nz = normaliser(B)
    evs = evaluators(B, nz)
    before = g.kernel_launches
    got = g.evaluate(evs)
    rounds = max(sum(p[0]) for p in PLANS)
    assert g.kernel_launches == before + rounds          # ONE acting launch per round, over the members with an open episode
    for m, member in enumerate(g.members):
        alone = evaluators(B, nz)[m]
        want = alone.evaluate(member)
        assert (f32_bits(got[m].score), f32_bits(got[m].normalized), got[m].n_steps, got[m].n_episodes) == \
               (f32_bits(want.score), f32_bits(want.normalized), want.n_steps, want.n_episodes), m
        assert evs[m].env.actions == alone.env.actions and len(alone.env.actions) == sum(PLANS[m][0]), m
        assert member.n_opts == 0
    assert got[1].normalized is not None and got[0].normalized is None
    g.close(); nz.close()


def test_an_evaluator_whose_action_row_is_not_the_members_is_refused(B):
    g = B.BcGroup.build([config(B, i) for i in range(2)])
    evs = [B.Evaluator(ScriptedEnv(m, [1]), 1, obs_dim=SHAPE[0], act_dim=SHAPE[1] + (m == 1), act_dtype=np.float32) for m in range(2)]
    with pytest.raises(B.BdrError, match="member 1"):
        g.evaluate(evs)
    assert g.kernel_launches == 0 and evs[0].env.actions == []
    g.close()


def files_under(root):
    out = {}
    for d, _, names in os.walk(root):
        for f in names:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


@pytest.mark.parametrize("form", ["general", "fused_mfma"])
def test_train_offline_with_post_processing_equals_the_standalone_twins(B, form, tmp_path):
    P, max_opts, record = 2, 6, 4
    plans = PLANS[:P]
    nz = normaliser(B)
    # the twins: bdr_trainer_train_offline_post of a lone agent
    want = []
    for i in range(P):
        a, rb, ev, events = B.Bc.build(config(B, i, form)), ring(B, 100 + i), evaluators(B, nz, plans)[i], []
        B.NativeTrainer(B.TrainerConfig(max_opts=max_opts, record_agent_info_interval=record)).train_offline(
            a, rb, on_event=lambda *e: events.append(e), evaluator=ev, eval_interval=2, save_interval=3, model_dir=str(tmp_path / f"twin{i}"))
        a.sync()
        want.append(({r: a.get_params(role=r) for r in ROLES}, a.n_opts, events, ev.env.actions, files_under(tmp_path / f"twin{i}")))
        a.close(); rb.close()
    g = B.BcGroup.build([config(B, i, form) for i in range(P)])
    rings, evs, events, records = [ring(B, 100 + i) for i in range(P)], evaluators(B, nz, plans), [], []
    stats = g.train_offline(rings, max_opts, record_interval=record, on_record=lambda k, r: records.append((k, r)), evaluators=evs, eval_interval=2,
                            save_interval=3, model_dirs=[str(tmp_path / f"group{i}") for i in range(P)], on_event=lambda *e: events.append(e))
    n_eval_launches = 3 * max(sum(p[0]) for p in plans)
    assert g.kernel_launches == max_opts * g.launches_per_round + n_eval_launches
    assert [k for k, _ in records] == [4] and all(s["opt_steps"] == max_opts and s["n_records"] == 1 for s in stats)
    for i, m in enumerate(g.members):
        params, n_opts, ev_twin, actions, files = want[i]
        for r in ROLES:
            assert np.array_equal(m.get_params(role=r), params[r]), (form, i, r)
        assert m.n_opts == n_opts == max_opts
        mine = [e[1:] for e in events if e[0] == i]
        assert [(e, o, n, [np.float32(x).tobytes() for x in sc]) for e, o, n, sc in mine] == \
               [(e, o, n, [np.float32(x).tobytes() for x in sc]) for e, o, n, sc in ev_twin], (form, i)
        assert [n for _, _, n, _ in mine] == ["opt", "opt", "eval", "opt", "opt_record", "eval", "opt", "opt", "eval"]
        assert np.float32(records[0][1][i]["loss"]) == np.float32(ev_twin[4][3][0])
        assert evs[i].env.actions == actions
        got_files = files_under(tmp_path / f"group{i}")
        assert got_files == files and {os.path.dirname(k) for k in files} == {"best", "3", "6"}, (form, i, sorted(got_files))
    g.close(); nz.close()
    for rb in rings: rb.close()
