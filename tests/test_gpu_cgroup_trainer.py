"""CandleSacGroup.train / AwacGroup.train (bdr_trainer_train_cgroup_post: the compiled online loop over a continuous-action group, with
post-processing) against NativeTrainer.train of each standalone TWIN - the same configs, seeds and environments, one run each.
P = 3, shape `one_action` (obs 3, act 1), max_opts 9, warmup_period 4, opt_interval 2, record_agent_info_interval 3, eval_interval 4
with a 2-episode evaluator, save_interval 5 into tmp dirs.  Equal member by member, bit for bit: the event sequence with its scalars,
the statistics, the rings, the arenas by role, the noise counter (trailing draws), the saved files (so the tensors and the `best`
model chosen) and the actions the evaluation environments saw.
The environments are scripted: rows from a seeded generator that depend on the action taken, episodes of 5 steps, one environment per
member.  They produce float64 values; `obs_dtype` says how the loop keeps them.  With np.float64 the group stages the raw rows and the
device rounds them once (acting and the grouped push alike); the twin's loop rounds the same values to float32 on the host, the same
cast, and acts and pushes float32 rows."""
import numpy as np
import pytest

from border_amd.trainer import NativeTrainer, Step, TrainerConfig
from tests import test_gpu_awac_group as TA
from tests import test_gpu_candle_sac_group as TC
from tests.test_gpu_candle_sac_group_eval import files_under
from tests.test_gpu_group_push import assert_same_ring, ring_state

pytestmark = pytest.mark.gpu

P = 3
CONFIG = dict(max_opts=9, warmup_period=4, opt_interval=2, record_agent_info_interval=3)
EVAL_INTERVAL, SAVE_INTERVAL, EPISODE = 4, 5, 5
KINDS = {
    "awac": (TA, "Awac", "AwacGroup", (3, 1, (64, 64), (64, 64), "None", 2, 34, ("Tanh", "Mse", False))),
    "candle_sac": (TC, "CandleSac", "CandleSacGroup", TC.SHAPES["one_action"]),
}


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


class ScriptedEnv:
    """Deterministic given the actions: float64 rows of a seeded generator shifted by the action, episodes of EPISODE steps whose last
    step terminates (even episodes) or truncates (odd ones); raises at step `fail_at`."""
    def __init__(self, od, seed, fail_at=None):
        self.od, self.rng, self.t, self.ep, self.n, self.fail_at = od, np.random.default_rng(seed), 0, 0, 0, fail_at

    def reset(self, _=None):
        self.t = 0
        return self.rng.standard_normal((1, self.od))

    def step_with_reset(self, act):
        self.n += 1
        if self.n == self.fail_at:
            raise RuntimeError(f"scripted failure at step {self.n}")
        a = float(np.asarray(act).reshape(-1)[0])
        self.t += 1
        obs = self.rng.standard_normal((1, self.od)) + 0.25 * a
        done = self.t == EPISODE
        term = done and self.ep % 2 == 0
        st = Step(np.asarray(act), obs, np.array([1.0 + 0.5 * a], np.float32), np.array([1 if term else 0], np.int8), np.array([1 if done and not term else 0], np.int8))
        if done:
            self.ep += 1
            st.init_obs = self.reset()
        return st


class EvalEnv:
    """the evaluation environment of member m: 2 episodes of 3 and 2 steps, the reward carries the action"""
    def __init__(self, od, m):
        self.od, self.m, self.ix, self.t, self.actions = od, m, 0, 0, []

    def obs(self):
        return 1.5 * np.sin(0.41 * np.arange(self.od, dtype=np.float64) + self.m + 2.0 * self.ix + 0.5 * self.t)

    def reset_with_index(self, ix):
        self.ix, self.t = ix, 0
        return self.obs()

    def step(self, act):
        self.actions.append((self.ix, self.t, act.tobytes()))
        self.t += 1
        done = self.t == (3, 2)[self.ix]
        return self.obs(), float(np.sum(act, dtype=np.float32)), done and self.ix == 0, done and self.ix == 1


def empty_ring(B, shape, seed):
    return B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=16, seed=seed), (shape[0],), np.float32, (shape[1],), np.float32, device=0)


def evaluator(B, shape, m, dtype):
    return B.Evaluator(EvalEnv(shape[0], m), 2, obs_dtype=dtype, obs_dim=shape[0], act_dim=shape[1], act_dtype=np.float32)


def bits(events):
    return [(e, o, name, [np.float32(x).tobytes() for x in sc]) for e, o, name, sc in events]


def result(mod, shape, a, rb, events, stats, ev, root):
    a.sync()
    return {"state": mod.state(a, rb, shape), "ring": ring_state(rb), "events": bits(events), "n_opts": a.n_opts, "actions": ev.env.actions,
            "stats": {k: stats[k] for k in ("env_steps", "opt_steps", "n_records", "n_episodes")}, "files": files_under(root)}


def twin(B, kind, i, dtype, root):
    """bdr_trainer_train_post of a lone agent; float64 environments: the loop keeps the rows as float32 (the same cast, on the host)"""
    mod, agent, _, shape = KINDS[kind]
    a, rb, ev, events = getattr(B, agent).build(mod.config(B, shape, i)), empty_ring(B, shape, 40 + i), evaluator(B, shape, i, dtype), []
    st = NativeTrainer(TrainerConfig(**CONFIG)).train(ScriptedEnv(shape[0], 300 + i), a, rb, (shape[0],), np.float32, act_row_bytes=4 * shape[1], act_dtype=np.float32,
                                                      on_event=lambda e, o, name, sc: events.append((e, o, name, sc)), evaluator=ev,
                                                      eval_interval=EVAL_INTERVAL, save_interval=SAVE_INTERVAL, model_dir=str(root))
    out = result(mod, shape, a, rb, events, st, ev, root)
    a.close(); rb.close()
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_the_group_loop_equals_the_loops_of_its_twins(B, kind, dtype, tmp_path):
    mod, _, group, shape = KINDS[kind]
    want = [twin(B, kind, i, dtype, tmp_path / f"twin{i}") for i in range(P)]
    g = getattr(B, group).build([mod.config(B, shape, i) for i in range(P)])
    bufs, evs, events = [empty_ring(B, shape, 40 + i) for i in range(P)], [evaluator(B, shape, i, dtype) for i in range(P)], [[] for _ in range(P)]
    dirs = [tmp_path / f"group{i}" for i in range(P)]
    stats = g.train([ScriptedEnv(shape[0], 300 + i) for i in range(P)], bufs, TrainerConfig(**CONFIG), obs_dtype=dtype,
                    on_event=lambda m, e, o, name, sc: events[m].append((e, o, name, sc)), evaluators=evs, eval_interval=EVAL_INTERVAL,
                    save_interval=SAVE_INTERVAL, model_dirs=dirs)
    n_iter = 4 + 2 * 8   # the first opt at env_steps 4, then every second step
    # one acting launch and one grouped push per iteration, the rounds, and the 2 evaluations' 5 acting rounds each (episodes of 3 and 2 steps)
    assert g.kernel_launches == 2 * n_iter + CONFIG["max_opts"] * g.launches_per_round + 2 * 5
    for i, (m, rb) in enumerate(zip(g.members, bufs)):
        got, w = result(mod, shape, m, rb, events[i], stats[i], evs[i], dirs[i]), want[i]
        assert got["events"] == w["events"], (i, got["events"], w["events"])
        assert [e[2] for e in got["events"] if e[2] != "skip"] == ["opt", "opt", "opt_record", "opt", "eval", "opt", "opt_record", "opt", "opt", "eval", "opt_record"]
        assert got["stats"] == w["stats"] == {"env_steps": n_iter, "opt_steps": 9, "n_records": 3, "n_episodes": n_iter // EPISODE}, (i, got["stats"], w["stats"])
        assert_same_ring(got["ring"], w["ring"], f"member {i}")
        mod.assert_same(got["state"], w["state"], (kind, i))
        assert got["n_opts"] == w["n_opts"] == 9
        assert got["actions"] == w["actions"] and len(got["actions"]) == 2 * 5, i
        assert got["files"] == w["files"], (i, sorted(got["files"]), sorted(w["files"]))
        assert {k.split("/")[0] for k in got["files"]} == {"best", "5"}, sorted(got["files"])
    g.close()
    for rb in bufs: rb.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_an_environments_exception_is_raised_again_and_the_group_stays_usable(B, kind):
    mod, _, group, shape = KINDS[kind]
    g = getattr(B, group).build([mod.config(B, shape, i) for i in range(P)])
    bufs = [empty_ring(B, shape, 40 + i) for i in range(P)]
    envs = [ScriptedEnv(shape[0], 300 + i, fail_at=7 if i == 1 else None) for i in range(P)]
    with pytest.raises(RuntimeError, match="scripted failure at step 7"):
        g.train(envs, bufs, TrainerConfig(**CONFIG))
    g.sync()
    assert [rb.len() for rb in bufs] == [6] * P and [e.n for e in envs] == [7, 7, 6]   # member 2 was not stepped any more, nothing of step 7 was pushed
    stats = g.train([ScriptedEnv(shape[0], 500 + i) for i in range(P)], bufs, TrainerConfig(max_opts=2, warmup_period=0, opt_interval=1))
    assert [s["opt_steps"] for s in stats] == [2] * P and [rb.len() for rb in bufs] == [8] * P
    g.close()
    for rb in bufs: rb.close()
