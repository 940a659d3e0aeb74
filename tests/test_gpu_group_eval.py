"""Acting for a subset of a group's members (bdr_agent_group_sample_members, DqnGroup.sample(members=...)), the lockstep evaluator
(bdr_evaluate_group, DqnGroup.evaluate) and Trainer::post_process in the group loop (bdr_trainer_train_group_post, DqnGroup.train with
evaluators) against standalone TWINS: the same configs, seeds, explorers and environments, one agent after the other through
Dqn.sample, Evaluator.evaluate and NativeTrainer.train(..., evaluator=...).  Every comparison is `==`."""
import os

import numpy as np
import pytest

from border_amd.evaluator import Evaluator
from border_amd.trainer import NativeTrainer, TrainerConfig
from tests.test_gpu_agent_group import ARENAS, clean_env, hetero
from tests.test_gpu_group_trainer import ToyEnv, result, ring_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


class EvalEnv:
    """The ToyEnv idea for an Evaluator: reset_with_index(ix) seeds the episode from (seed, ix) - 5..9 steps, observations and rewards
    that depend on the action taken, a terminal or a truncating last step."""
    def __init__(self, in_dim, seed):
        self.in_dim, self.seed, self.rng, self.left = in_dim, seed, None, 0

    def reset_with_index(self, ix):
        self.rng = np.random.default_rng([self.seed, ix])
        self.left = int(self.rng.integers(5, 10))
        return self.rng.standard_normal(self.in_dim).astype(np.float32)

    def step(self, act):
        a = int(np.asarray(act).reshape(-1)[0])
        self.left -= 1
        obs = (self.rng.standard_normal(self.in_dim) + 0.25 * a).astype(np.float32)
        reward = float(np.float32(1.0 + 0.5 * a + self.rng.random()))
        done = self.left == 0
        trunc = done and bool(self.rng.random() < 0.5)
        return obs, reward, done and not trunc, trunc


def prepare(B, i, agent, train=True):
    agent.set_explorer(B.EpsilonGreedy(final_step=40), seed=70 + i)
    agent.train() if train else agent.eval()


def evaluator(in_dim, seed, n_episodes, ref_scores=None):
    return Evaluator(EvalEnv(in_dim, seed), n_episodes, obs_dim=in_dim, act_dim=1, act_dtype=np.int64, ref_scores=ref_scores)


def same_result(got, want, what):
    assert np.float32(got.score).tobytes() == np.float32(want.score).tobytes(), (what, got, want)
    assert (got.normalized is None) == (want.normalized is None), what
    if want.normalized is not None:
        assert np.float32(got.normalized).tobytes() == np.float32(want.normalized).tobytes(), (what, got, want)
    assert (got.n_steps, got.n_episodes) == (want.n_steps, want.n_episodes), (what, got, want)


SCHEDULE = [[0, 1, 2, 3, 4], [0], [4], [1, 3], [2], None]   # None: the full call, through the existing entry


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_subset_acting_equals_the_twins(B, train, monkeypatch):
    clean_env(monkeypatch)
    members = hetero(B, 1)
    P = len(members)
    dims = [c.model_config.q_config.in_dim for c, _ in members]
    rng = np.random.default_rng(21)
    calls = [(sel, [rng.standard_normal(d).astype(np.float32) for d in dims]) for sel in SCHEDULE * 4]   # 24 calls: the eps schedule moves
    last = [rng.standard_normal(d).astype(np.float32) for d in dims]
    # twins: a twin is sampled only when its member is selected
    want, want_last, want_q = [[] for _ in members], [], []
    for i, (c, _) in enumerate(members):
        a = B.Dqn.build(c)
        prepare(B, i, a, train)
        for sel, rows in calls:
            if sel is None or i in sel:
                act, info = a.sample(rows[i][None], return_info=True)
                want[i].append((int(act[0]), info))
            else:
                want[i].append(None)
        act, info = a.sample(last[i][None], return_info=True)
        want_last.append((int(act[0]), info))
        want_q.append(a.qvalues(last[i][None])[0])
        a.close()
    # the group
    g = B.DqnGroup.build([c for c, _ in members])
    for i, m in enumerate(g.members): prepare(B, i, m, train)
    n_random = 0
    for k, (sel, rows) in enumerate(calls):
        act, info = g.sample(rows, return_info=True, members=sel)
        for i in range(P):
            if want[i][k] is None: continue
            assert (int(act[i]), info[i]) == want[i][k], (k, i)
            n_random += info[i]["is_random"]
    if train: assert n_random > 0
    # every refusal moves nothing: the next full call still equals the twins'
    for bad in ([], [5], [3, 1], [2, 2]):
        with pytest.raises(B.BdrError):
            g.sample(last, members=bad)
    act, info = g.sample(last, return_info=True)
    for i in range(P):
        assert (int(act[i]), info[i]) == want_last[i], i
    for i, q in enumerate(g.qvalues(last)):
        assert q.shape == want_q[i].shape and (q == want_q[i]).all(), i
    g.close()


N_EPISODES = [1, 3, 2]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_group_evaluate_equals_evaluator_on_twins(B, train, monkeypatch):
    clean_env(monkeypatch)
    h = hetero(B, 1)
    members = [h[0], h[2], h[3]]   # in_dim 4, 3, 6
    dims = [c.model_config.q_config.in_dim for c, _ in members]
    refs = [None, (-2.5, 31.0), None]
    fresh = [np.random.default_rng(5).standard_normal(d).astype(np.float32) for d in dims]
    want, want_next = [], []
    for i, (c, _) in enumerate(members):
        a = B.Dqn.build(c)
        prepare(B, i, a, train)
        want.append(evaluator(dims[i], 500 + i, N_EPISODES[i], refs[i]).evaluate(a))
        act, info = a.sample(fresh[i][None], return_info=True)
        want_next.append((int(act[0]), info))
        a.close()
    g = B.DqnGroup.build([c for c, _ in members])
    for i, m in enumerate(g.members): prepare(B, i, m, train)
    got = g.evaluate([evaluator(dims[i], 500 + i, N_EPISODES[i], refs[i]) for i in range(3)])
    for i in range(3):
        same_result(got[i], want[i], i)
        assert got[i].n_episodes == N_EPISODES[i]
    assert got[1].normalized is not None and got[0].normalized is None
    assert len({r.n_steps for r in got}) == 3   # the members finished on different rounds: the subset launch was exercised
    act, info = g.sample(fresh, return_info=True)   # the explorer streams and counters ended where the twins' did
    for i in range(3):
        assert (int(act[i]), info[i]) == want_next[i], i
    assert [m.is_train() for m in g.members] == [train] * 3   # the mode is not touched
    g.close()


CONFIG = dict(warmup_period=20, opt_interval=2, record_agent_info_interval=5, max_opts=12)


def saved(B, c, d):
    a = B.Dqn.build(c)
    a.load_params(d)
    out = {k: a.get_params(k) for k in ("qnet", "qnet_tgt")}
    a.close()
    return out


def test_group_train_with_post_processing_equals_the_twins(B, tmp_path, monkeypatch):
    clean_env(monkeypatch)
    h = hetero(B, 1)
    members = [h[0], h[2], h[3]]
    dims = [c.model_config.q_config.in_dim for c, _ in members]
    refs = [None, (-2.5, 31.0), None]
    post = dict(eval_interval=4, save_interval=6)
    want = []
    for i, (c, seed) in enumerate(members):
        a, rb = B.Dqn.build(c), ring_of(B, c, seed)
        a.set_explorer(B.EpsilonGreedy(final_step=40), seed=70 + i)
        ev = []
        st = NativeTrainer(TrainerConfig(**CONFIG)).train(ToyEnv(dims[i], 300 + i), a, rb, (dims[i],), np.float32,
                                                          on_event=lambda e, o, name, sc: ev.append((e, o, name, sc)),
                                                          evaluator=evaluator(dims[i], 500 + i, N_EPISODES[i], refs[i]),
                                                          model_dir=str(tmp_path / f"twin{i}"), **post)
        want.append(result(a, rb, ev, st))
        a.close(); rb.close()
    g = B.DqnGroup.build([c for c, _ in members])
    for i, m in enumerate(g.members): m.set_explorer(B.EpsilonGreedy(final_step=40), seed=70 + i)
    bufs = [ring_of(B, c, seed) for c, seed in members]
    events = [[] for _ in members]
    stats = g.train([ToyEnv(d, 300 + i) for i, d in enumerate(dims)], bufs, TrainerConfig(**CONFIG),
                    on_event=lambda m, e, o, name, sc: events[m].append((e, o, name, sc)),
                    evaluators=[evaluator(dims[i], 500 + i, N_EPISODES[i], refs[i]) for i in range(3)],
                    model_dirs=[str(tmp_path / f"member{i}") for i in range(3)], **post)
    g.sync()
    got = [result(m, rb, events[i], stats[i]) for i, (m, rb) in enumerate(zip(g.members, bufs))]
    for i, (gt, w) in enumerate(zip(got, want)):
        for k in ARENAS:
            assert (gt["arenas"][k] == w["arenas"][k]).all(), (i, k)
        assert gt["len"] == w["len"] and gt["head"] == w["head"], i
        for a, b in zip(gt["rows"], w["rows"]):
            assert (a.view(np.uint8) == b.view(np.uint8)).all(), i
        assert (gt["ixs"] == w["ixs"]).all(), i
        assert gt["stats"] == w["stats"], (i, gt["stats"], w["stats"])
        assert gt["events"] == w["events"], (i, gt["events"], w["events"])
        evals = [e for e in gt["events"] if e[2] == "eval"]
        assert [e[1] for e in evals] == [4, 8, 12] and all(len(e[3]) == (2 if refs[i] else 1) for e in evals), i
        assert gt["n_opts"] == w["n_opts"] == 12
        mine, twin = str(tmp_path / f"member{i}"), str(tmp_path / f"twin{i}")
        assert sorted(os.listdir(mine)) == sorted(os.listdir(twin)) == ["12", "6", "best"], i
        for d in ("best", "6", "12"):
            a, b = saved(B, members[i][0], os.path.join(mine, d)), saved(B, members[i][0], os.path.join(twin, d))
            for k in ("qnet", "qnet_tgt"):
                assert (a[k] == b[k]).all(), (i, d, k)
    g.close()
    for rb in bufs: rb.close()


@pytest.mark.parametrize("prioritized", [False, True], ids=["group_of_one", "prioritized_pair"])
def test_a_group_of_one_and_a_prioritized_group(B, prioritized, monkeypatch):
    from tests.test_gpu_group_per import PRing
    clean_env(monkeypatch)
    h = hetero(B, 1)
    members = [h[0], h[2]] if prioritized else [h[3]]
    per = (700, 0.6, "All") if prioritized else None
    dims = [c.model_config.q_config.in_dim for c, _ in members]
    n_eps = [2, 1]
    want = []
    for i, (c, seed) in enumerate(members):
        a, ring = B.Dqn.build(c), PRing(B, c, seed, per)
        prepare(B, i, a)
        a.opt(ring.rb)
        want.append(evaluator(dims[i], 900 + i, n_eps[i]).evaluate(a))
        a.close(); ring.rb.close()
    g = B.DqnGroup.build([c for c, _ in members], prioritized=prioritized)
    rings = [PRing(B, c, seed, per) for c, seed in members]
    for i, m in enumerate(g.members): prepare(B, i, m)
    g.opt([r.rb for r in rings])
    got = g.evaluate([evaluator(dims[i], 900 + i, n_eps[i]) for i in range(len(members))])
    for i in range(len(members)):
        same_result(got[i], want[i], i)
    g.close()
    for r in rings: r.rb.close()
