"""bdr_trainer_train_group (DqnGroup.train): the compiled online loop over a group against bdr_trainer_train on standalone TWINS -
the same configs, seeds, explorers and environments, one run each.  Per member: equal arenas, ring rows, counters, observer events
and Record scalars, all with `==`."""
import numpy as np
import pytest

from border_amd.trainer import NativeTrainer, Step, TrainerConfig
from tests.test_gpu_agent_group import ARENAS, clean_env, hetero

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


class ToyEnv:
    """Seeded and deterministic given the actions: episodes of 5..9 steps (drawn per episode), observations that depend on the action
    taken, a terminal or a truncating last step."""
    def __init__(self, in_dim, seed):
        self.in_dim, self.rng, self.left = in_dim, np.random.default_rng(seed), 0

    def reset(self, _=None):
        self.left = int(self.rng.integers(5, 10))
        return self.rng.standard_normal((1, self.in_dim)).astype(np.float32)

    def step_with_reset(self, act):
        a = int(np.asarray(act).reshape(-1)[0])
        self.left -= 1
        obs = (self.rng.standard_normal((1, self.in_dim)) + 0.25 * a).astype(np.float32)
        done = self.left == 0
        trunc = done and bool(self.rng.random() < 0.5)
        st = Step(np.asarray(act), obs, np.array([1.0 + 0.5 * a], np.float32), np.array([1 if done and not trunc else 0], np.int8),
                  np.array([1 if trunc else 0], np.int8))
        if done:
            st.init_obs = self.reset()
        return st


CONFIG = dict(warmup_period=20, opt_interval=2, record_agent_info_interval=5, max_opts=30)


def prepare(B, i, agent):
    agent.set_explorer(B.EpsilonGreedy(final_step=40), seed=70 + i)


def ring_of(B, c, seed):
    return B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=seed), (c.model_config.q_config.in_dim,), np.float32)


def result(agent, rb, events, stats):
    agent.sync()
    n = rb.len()
    return {"arenas": {k: agent.get_params(k) for k in ARENAS}, "rows": rb.read_rows(0, n), "len": n, "head": rb.head,
            "ixs": rb.sample_indices(40), "events": events, "n_opts": agent.n_opts,
            "stats": {k: stats[k] for k in ("env_steps", "opt_steps", "n_records", "n_episodes")}}


@pytest.mark.parametrize("n_upd", [1, 2])
def test_group_loop_equals_three_single_loops(B, n_upd, monkeypatch):
    clean_env(monkeypatch)
    h = hetero(B, n_upd)
    members = [h[0], h[2], h[3]]   # in_dim 4, 3, 6; batch 32, 17, 32
    dims = [c.model_config.q_config.in_dim for c, _ in members]
    # twins: bdr_trainer_train, one member at a time
    want = []
    for i, (c, seed) in enumerate(members):
        a, rb = B.Dqn.build(c), ring_of(B, c, seed)
        prepare(B, i, a)
        ev = []
        st = NativeTrainer(TrainerConfig(**CONFIG)).train(ToyEnv(dims[i], 300 + i), a, rb, (dims[i],), np.float32,
                                                          on_event=lambda e, o, name, sc: ev.append((e, o, name, sc)))
        want.append(result(a, rb, ev, st))
        a.close(); rb.close()
    # the group
    g = B.DqnGroup.build([c for c, _ in members])
    for i, m in enumerate(g.members): prepare(B, i, m)
    bufs = [ring_of(B, c, seed) for c, seed in members]
    events = [[] for _ in members]
    stats = g.train([ToyEnv(d, 300 + i) for i, d in enumerate(dims)], bufs, TrainerConfig(**CONFIG),
                    on_event=lambda m, e, o, name, sc: events[m].append((e, o, name, sc)))
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
        assert gt["events"] == w["events"], i
        assert gt["n_opts"] == w["n_opts"] == 30
        assert gt["stats"]["opt_steps"] == 30 and gt["stats"]["n_records"] == 6 and gt["stats"]["env_steps"] == 78
        assert sum(1 for e in gt["events"] if e[2] == "opt_record" and len(e[3]) > 0) == 6
    assert len({tuple(g_["rows"][4].tolist()) for g_ in got}) == 3   # the members' episodes end on different iterations
    g.close()
    for rb in bufs: rb.close()
