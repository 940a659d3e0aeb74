"""The compiled Evaluator (csrc/trainer.hip: bdr_evaluate) and the Trainer's post-processing (bdr_trainer_train_post /
bdr_trainer_train_offline_post) against border-core/src/evaluator/default_evaluator.rs:64-88 and trainer.rs:231-264, driven with
mock agent / environment / save callbacks - no GPU involved."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from border_amd import _lib
from border_amd.evaluator import Evaluator
from border_amd.trainer import NativeTrainer, TrainerConfig

sys.path.insert(0, os.path.dirname(__file__))
from test_native_trainer import MockAgentBuffer, MockEnv  # noqa: E402

F32_MIN = -float(np.finfo(np.float32).max)


class ScriptEnv:
    """Episodes given as lists of (reward, is_terminated, is_truncated); the observation is [ix, t, 0, 0] f32.  `episodes` is a
    callable ix -> list so that an environment can hand out different episodes evaluation after evaluation."""
    def __init__(self, episodes):
        self.episodes = episodes if callable(episodes) else (lambda ix: episodes[ix])
        self.log, self.cur, self.t, self.ix = [], None, 0, -1

    def reset_with_index(self, ix):
        self.log.append(("reset", ix))
        self.cur, self.t, self.ix = self.episodes(ix), 0, ix
        return np.array([ix, 0, 0, 0], np.float32)

    def step(self, act):
        r, term, trunc = self.cur[self.t]
        self.t += 1
        self.log.append(("step", self.ix, self.t, int(act[0])))
        return np.array([self.ix, self.t, 0, 0], np.float32), r, term, trunc


def mock_evaluator(env, n_episodes, log, ref_scores=None):
    """an Evaluator over `env` whose agent hook is a mock: the action is the number of sample calls so far"""
    ev = Evaluator(env, n_episodes, obs_dim=4, act_dim=1, act_dtype=np.int64, ref_scores=ref_scores)
    c = ev.c_struct()
    n = {"k": 0}

    def sample(_a, n_procs, obs, act_out):
        o = np.frombuffer((C.c_char * 16).from_address(obs), np.float32).copy()
        n["k"] += 1
        log.append(("sample", int(o[0]), int(o[1])))
        C.cast(act_out, C.POINTER(C.c_int64))[0] = n["k"]
        return 0

    ev._sample = _lib.SAMPLE_FN(sample)
    c.agent_sample = ev._sample
    return ev


def evaluate(ev):
    out = _lib.EvalResultC()
    _lib.check(_lib.lib().bdr_evaluate(C.byref(ev.c_struct()), None, C.byref(out)))
    return out


def test_episode_loop_order_and_both_ways_an_episode_ends():
    eps = [[(1.0, 0, 0), (2.0, 1, 0), (100.0, 0, 0)],            # ends by termination at its second step (the third is never taken)
           [(0.5, 0, 0), (0.25, 0, 0), (0.125, 0, 1)],           # ends by truncation
           [(4.0, 1, 1)]]
    env, log = ScriptEnv(eps), []
    ev = mock_evaluator(env, 3, log)
    out = evaluate(ev)
    assert [x for x in env.log if x[0] == "reset"] == [("reset", 0), ("reset", 1), ("reset", 2)]
    assert [x[1:3] for x in env.log if x[0] == "step"] == [(0, 1), (0, 2), (1, 1), (1, 2), (1, 3), (2, 1)]
    # Policy::sample sees reset_with_index's row first, then step.obs; one sample per step, its action handed to that step
    assert log == [("sample", 0, 0), ("sample", 0, 1), ("sample", 1, 0), ("sample", 1, 1), ("sample", 1, 2), ("sample", 2, 0)]
    assert [x[3] for x in env.log if x[0] == "step"] == [1, 2, 3, 4, 5, 6]
    assert (out.n_steps, out.n_episodes) == (6, 3)
    assert out.score == np.float32(np.float32(7.875) / np.float32(3))
    assert out.has_normalized == 0


def test_the_score_is_one_f32_accumulator_in_call_order():
    rewards = [1e8, 1.0, -1e8, 0.5, 0.25, 0.25, 0.25, 0.25]   # f32: 1e8 + 1 = 1e8, so the 1 is lost: 1.5; float64: 2.5
    eps = [[(r, 0, 0) for r in rewards[:3]] + [(rewards[3], 1, 0)], [(r, 0, 0) for r in rewards[4:7]] + [(rewards[7], 0, 1)]]
    out = evaluate(mock_evaluator(ScriptEnv(eps), 2, []))
    acc = np.float32(0)
    for r in rewards:
        acc = np.float32(acc + np.float32(r))
    want = np.float32(acc / np.float32(2))
    assert float(sum(rewards)) / 2 != float(want)          # float64 accumulation gives another number: the order and the width matter
    assert out.score == want == np.float32(0.75)


def test_normalized_score():
    eps = [[(3.0, 1, 0)], [(4.5, 0, 1)]]
    out = evaluate(mock_evaluator(ScriptEnv(eps), 2, [], ref_scores=(-1.5, 9.25)))
    score = np.float32(np.float32(7.5) / np.float32(2))
    assert out.score == score and out.has_normalized == 1
    assert out.normalized == np.float32((score - np.float32(-1.5)) / (np.float32(9.25) - np.float32(-1.5)))
    res = mock_evaluator(ScriptEnv(eps), 2, []).evaluate(type("A", (), {"handle": None})())
    assert res.score == score and res.normalized is None


def test_argument_checks():
    from border_amd import BdrError
    ev = mock_evaluator(ScriptEnv([[(1.0, 1, 0)]]), 0, [])
    with pytest.raises(BdrError):
        evaluate(ev)
    m = MockAgentBuffer()
    with pytest.raises(BdrError):   # an eval interval without an evaluator
        NativeTrainer(TrainerConfig(max_opts=2)).train_offline(None, None, ops=m.ops(), eval_interval=1, model_dir="/nonexistent")
    with pytest.raises(BdrError):   # a save interval without a directory
        NativeTrainer(TrainerConfig(max_opts=2)).train_offline(None, None, ops=m.ops(), save_interval=1)


class Saves:
    def __init__(self):
        self.dirs = []
        self.fn = _lib.SAVE_FN(lambda _a, d: (self.dirs.append(d.decode()), 0)[1])


def run_post(scores, max_opts, eval_interval, save_interval, online=False, cfg=None):
    """the loop with a mock evaluator whose k-th evaluation scores scores[k] (one episode of one step with that reward)"""
    k = {"n": -1}

    def episodes(ix):
        k["n"] += 1
        return [(scores[k["n"]], 1, 0)]

    m, saves, events, elog = MockAgentBuffer(), Saves(), [], []
    ops = m.ops()
    ev = mock_evaluator(ScriptEnv(episodes), 1, elog)
    # the evaluation's sample calls go through the evaluator's own hook: mark them in the agent's log to see them between set_train calls
    inner = ev._sample

    def sample(a, n, obs, act):
        m.log.append(("eval_sample",))
        return inner(a, n, obs, act)
    ev._sample2 = _lib.SAMPLE_FN(sample)
    ev.c_struct().agent_sample = ev._sample2
    nt = NativeTrainer(TrainerConfig(max_opts=max_opts, **(cfg or {})))
    on_event = lambda e, o, name, sc: events.append((e, o, name, sc))
    kw = dict(on_event=on_event, ops=ops, evaluator=ev, eval_interval=eval_interval, save_interval=save_interval, model_dir="/models/run", save_params=saves.fn)
    st = nt.train(MockEnv(), None, None, (4,), np.float32, **kw) if online else nt.train_offline(None, None, **kw)
    return m, saves, events, st


def test_post_processing_over_twelve_opt_steps():
    m, saves, events, st = run_post([1.0, 3.0, 3.0], 12, 4, 5)
    assert st["opt_steps"] == 12
    evals = [(o, sc) for _, o, name, sc in events if name == "eval"]
    assert evals == [(4, [1.0]), (8, [3.0]), (12, [3.0])]
    # every evaluation is bracketed by eval() / train() (trainer.rs:246-248), whatever the score
    kinds = [x for x in m.log if x[0] in ("train", "eval_sample")]
    assert kinds == [("train", 1)] + [("train", 0), ("eval_sample",), ("train", 1)] * 3
    # best at 4 (1 > f32::MIN) and 8 (3 > 1), not at 12 (3 > 3 is false); numbered saves at 5 and 10; in loop order
    assert saves.dirs == ["/models/run/best", "/models/run/5", "/models/run/best", "/models/run/10"]
    # the event stream: the opt event of a step, then its eval event
    names = [(o, name) for _, o, name, _ in events]
    assert names.index((4, "eval")) == names.index((4, "opt")) + 1 and names.index((5, "opt")) == names.index((4, "eval")) + 1
    # where in the agent's call sequence the evaluations sit: after the 4th, 8th and 12th opt
    seq = [x[0] for x in m.log if x[0] in ("opt", "eval_sample")]
    assert seq == ["opt"] * 4 + ["eval_sample"] + ["opt"] * 4 + ["eval_sample"] + ["opt"] * 4 + ["eval_sample"]


def test_eval_event_carries_the_normalized_score_with_reference_scores():
    m, events, elog = MockAgentBuffer(), [], []
    ev = mock_evaluator(ScriptEnv(lambda ix: [(2.0, 0, 1)]), 1, elog, ref_scores=(1.0, 5.0))
    saves = Saves()
    NativeTrainer(TrainerConfig(max_opts=2)).train_offline(None, None, ops=m.ops(), on_event=lambda e, o, n, sc: events.append((o, n, sc)),
                                                           evaluator=ev, eval_interval=2, model_dir="/d", save_params=saves.fn)
    assert [x for x in events if x[1] == "eval"] == [(2, "eval", [2.0, 0.25])]
    assert saves.dirs == ["/d/best"]


def test_interval_zero_means_never():
    m, saves, events, st = run_post([], 6, 0, 0)
    assert st["opt_steps"] == 6 and saves.dirs == [] and not [e for e in events if e[2] == "eval"]
    assert [x for x in m.log if x[0] == "train"] == [("train", 1)]
    m, saves, events, _ = run_post([], 6, 0, 4)              # saves alone
    assert saves.dirs == ["/models/run/4"] and not [e for e in events if e[2] == "eval"]
    m, saves, events, _ = run_post([2.0, 1.0, 5.0], 6, 2, 0)  # evaluations alone
    assert saves.dirs == ["/models/run/best", "/models/run/best"] and [o for _, o, n, _ in events if n == "eval"] == [2, 4, 6]


def test_the_first_evaluation_is_always_saved_as_best():
    m, saves, events, _ = run_post([-3e38, -3.1e38], 2, 1, 0)
    assert saves.dirs == ["/models/run/best"]                # -3e38 > f32::MIN; the second, lower one is not saved
    assert [sc for _, _, n, sc in events if n == "eval"] == [[float(np.float32(-3e38))], [float(np.float32(-3.1e38))]]


def test_online_loop_post_processes_only_iterations_with_an_opt_step():
    cfg = dict(opt_interval=3, warmup_period=4)
    m, saves, events, st = run_post([1.0, 0.5], 4, 2, 1, online=True, cfg=cfg)
    assert st["opt_steps"] == 4 and st["env_steps"] == 15
    # opt steps at env steps 6, 9, 12, 15; opt_steps stays 2 over env steps 10 and 11 (2 % 2 == 0 there too): one evaluation per opt step
    evals = [(e, o) for e, o, n, _ in events if n == "eval"]
    assert evals == [(9, 2), (15, 4)]
    assert saves.dirs == ["/models/run/1", "/models/run/best", "/models/run/2", "/models/run/3", "/models/run/4"]
    # the environment steps of the evaluation are not the Trainer's: its own sample / push sequence is untouched
    assert [x[0] for x in m.log].count("sample") == 15 and [x[0] for x in m.log].count("push") == 15
    skips = [e for e, _, n, _ in events if n == "skip"]
    assert len(skips) == 11


@pytest.mark.parametrize("online", [False, True])
def test_post_null_reproduces_the_existing_entry(online):
    cfg = dict(max_opts=9, opt_interval=2, warmup_period=3, record_agent_info_interval=4, record_compute_cost_interval=3)

    def run(post):
        m, events = MockAgentBuffer(), []
        ops = m.ops()
        nt = NativeTrainer(TrainerConfig(**cfg))
        c, st = nt._config(16 if online else 0, 8 if online else 0), _lib.TrainerStatsC()
        obs = nt._observer(lambda e, o, name, sc: events.append((e, o, name, sc if name != "cost" else len(sc))))
        L = _lib.lib()
        if online:
            env = MockEnv()

            def reset(_c, out):
                C.memmove(out, env.reset(None).ctypes.data, 16); return 0

            def step(_c, act, out, reward, term, trunc, init_out):
                s = env.step_with_reset(np.zeros(1, np.int64))
                C.memmove(out, s.obs.ctypes.data, 16)
                reward[0], term[0], trunc[0] = float(s.reward[0]), int(s.is_terminated[0]), 0
                if s.is_done():
                    C.memmove(init_out, s.init_obs.ctypes.data, 16)
                return 0
            vt = _lib.EnvVtable(None, _lib.ENV_RESET_FN(reset), _lib.ENV_STEP_FN(step))
            rc = (L.bdr_trainer_train_post(C.byref(c), C.byref(ops), C.byref(vt), None, obs, None, C.byref(st)) if post
                  else L.bdr_trainer_train(C.byref(c), C.byref(ops), C.byref(vt), obs, None, C.byref(st)))
        else:
            rc = (L.bdr_trainer_train_offline_post(C.byref(c), C.byref(ops), None, obs, None, C.byref(st)) if post
                  else L.bdr_trainer_train_offline(C.byref(c), C.byref(ops), obs, None, C.byref(st)))
        assert rc == 0
        return events, m.log, m.pushed, (st.env_steps, st.opt_steps, st.n_records, st.n_episodes)

    assert run(True) == run(False)


def test_a_failing_environment_stops_the_evaluation_and_the_loop():
    class Boom(ScriptEnv):
        def step(self, act):
            raise RuntimeError("boom")
    ev = mock_evaluator(Boom([[(1.0, 1, 0)]]), 1, [])
    with pytest.raises(RuntimeError, match="boom"):
        ev.evaluate(type("A", (), {"handle": None})())
    m, saves = MockAgentBuffer(), Saves()
    with pytest.raises(RuntimeError, match="boom"):
        NativeTrainer(TrainerConfig(max_opts=5)).train_offline(None, None, ops=m.ops(), evaluator=ev, eval_interval=2, model_dir="/d", save_params=saves.fn)
    assert [x[0] for x in m.log].count("opt") == 2 and saves.dirs == []
