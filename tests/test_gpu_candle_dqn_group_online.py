"""The online half of a CandleDqnGroup against twins, every comparison == on bytes:
  push      bdr_candle_dqn_group_push (ONE launch of k_cgroup_push for all members, i64 action rows) of n = 1 and n = 5 rows per member
            into rings of capacity 3 - so n = 5 wraps the ring inside one push - against `rb.push` of the same rows as float32; even
            members push float32 rows, odd members float64 rows (converted on the device)
  train     bdr_trainer_train_group_post behind bdr_candle_dqn_group_trainer_ops_default / _trainer_post_default over scripted Python
            environments, P = 3, against NativeTrainer.train of every twin alone: parameters, ring bytes, index streams, events,
            statistics, scores and the saved files (qnet.pt / qnet_tgt.pt in model_dir/best and model_dir/<opt_steps>)
  evaluate  bdr_evaluate_group behind bdr_candle_dqn_group_eval_ops_default against Evaluator.evaluate member after member"""
import os

import numpy as np
import pytest

from border_amd.evaluator import Evaluator
from border_amd.trainer import NativeTrainer, TrainerConfig
from tests.test_gpu_candle_dqn_group import SHAPES, bits, config
from tests.test_gpu_group_eval import EvalEnv, same_result
from tests.test_gpu_group_push import assert_same_ring, ring_state
from tests.test_gpu_group_trainer import ToyEnv

pytestmark = pytest.mark.gpu

P = 3
SHAPE = SHAPES["cartpole_small"]   # obs 4, 2 actions, [64, 64], batch 64


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def empty_ring(B, seed, capacity):
    return B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed), (SHAPE[0],), np.float32, (1,), np.int64, device=0)


def draw(rng, n, dtype):
    od, A = SHAPE[0], SHAPE[1]
    return (rng.standard_normal((n, od)).astype(dtype), rng.integers(0, A, n).astype(np.int64), rng.standard_normal((n, od)).astype(dtype),
            rng.standard_normal(n).astype(np.float32), (rng.random(n) < .2).astype(np.int8), (rng.random(n) < .1).astype(np.int8))


@pytest.mark.parametrize("members", [1, 5])
def test_every_push_leaves_the_rings_as_a_standalone_push_does(B, members):
    g = B.CandleDqnGroup.build([config(B, SHAPE, i) for i in range(members)])
    bufs = [empty_ring(B, 20 + i, 3) for i in range(members)]
    twins = [empty_ring(B, 20 + i, 3) for i in range(members)]
    rngs = [np.random.default_rng(50 + i) for i in range(members)]
    launches = g.kernel_launches
    for k, n in enumerate([1, 1, 5, 1, 5, 5, 1, 1, 1, 1, 5, 1]):      # more pushes than the staging ring has slots (8)
        cols = [draw(rngs[i], n, np.float32 if i % 2 == 0 else np.float64) for i in range(members)]
        g.push([c[0] for c in cols], [c[1] for c in cols], [c[2] for c in cols], [c[3] for c in cols], [c[4] for c in cols], [c[5] for c in cols], buffers=bufs)
        launches += 1
        assert g.kernel_launches == launches, k
        for i in range(members):
            c = cols[i]
            twins[i].push(c[0].astype(np.float32), c[1], c[2].astype(np.float32), *c[3:])
            assert_same_ring(ring_state(bufs[i]), ring_state(twins[i]), (k, n, f"member {i}"))
    assert g.push_max_rows(buffers=bufs) > 5
    g.close()
    for rb in bufs + twins: rb.close()


CONFIG = dict(warmup_period=20, opt_interval=2, record_agent_info_interval=5, max_opts=12)
N_EPISODES = [1, 3, 2]
REFS = [None, (-2.5, 31.0), None]
POST = dict(eval_interval=4, save_interval=6)


def online_config(B, i):
    ex = B.EpsilonGreedy(eps_start=1.0, eps_final=0.1, final_step=40) if i != 1 else B.Softmax()
    return config(B, SHAPE, i, train=True, explorer=ex, batch_size=16)


def evaluator(i):
    return Evaluator(EvalEnv(SHAPE[0], 500 + i), N_EPISODES[i], obs_dim=SHAPE[0], act_dim=1, act_dtype=np.int64, ref_scores=REFS[i])


def result(agent, rb, events, stats):
    agent.sync()
    return {"arenas": {k: agent.get_params(*k) for k in (("qnet",), ("qnet_tgt",), ("qnet", "exp_avg"), ("qnet", "exp_avg_sq"))}, "ring": ring_state(rb),
            "events": [e for e in events if e[2] != "cost"], "n_opts": agent.n_opts,
            "stats": {k: stats[k] for k in ("env_steps", "opt_steps", "n_records", "n_episodes")}}


def saved(B, i, d):
    a = B.CandleDqn.build(online_config(B, i))
    a.load_params(d)
    out = {k: a.get_params(k) for k in ("qnet", "qnet_tgt")}
    a.close()
    return out


def event_bits(events):
    return [(e, o, name, [np.float32(v).view(np.uint32) for v in sc]) for e, o, name, sc in events]


def test_the_compiled_group_loop_with_post_processing_equals_the_twins(B, tmp_path):
    want = []
    for i in range(P):
        a, rb, ev = B.CandleDqn.build(online_config(B, i)), empty_ring(B, 30 + i, 64), []
        st = NativeTrainer(TrainerConfig(**CONFIG)).train(ToyEnv(SHAPE[0], 300 + i), a, rb, (SHAPE[0],), np.float32,
                                                          on_event=lambda e, o, name, sc: ev.append((e, o, name, sc)),
                                                          evaluator=evaluator(i), model_dir=str(tmp_path / f"twin{i}"), **POST)
        want.append(result(a, rb, ev, st))
        a.close(); rb.close()
    g = B.CandleDqnGroup.build([online_config(B, i) for i in range(P)])
    bufs = [empty_ring(B, 30 + i, 64) for i in range(P)]
    events = [[] for _ in range(P)]
    stats = g.train([ToyEnv(SHAPE[0], 300 + i) for i in range(P)], bufs, TrainerConfig(**CONFIG),
                    on_event=lambda m, e, o, name, sc: events[m].append((e, o, name, sc)),
                    evaluators=[evaluator(i) for i in range(P)], model_dirs=[str(tmp_path / f"member{i}") for i in range(P)], **POST)
    g.sync()
    for i in range(P):
        got, w = result(g.members[i], bufs[i], events[i], stats[i]), want[i]
        for k in w["arenas"]:
            assert (bits(got["arenas"][k]) == bits(w["arenas"][k])).all(), (i, k)
        assert_same_ring(got["ring"], w["ring"], f"member {i}")
        assert got["stats"] == w["stats"], (i, got["stats"], w["stats"])
        assert event_bits(got["events"]) == event_bits(w["events"]), i
        evals = [e for e in got["events"] if e[2] == "eval"]
        assert [e[1] for e in evals] == [4, 8, 12] and all(len(e[3]) == (2 if REFS[i] else 1) for e in evals), i
        assert got["n_opts"] == w["n_opts"] == 12
        mine, twin = str(tmp_path / f"member{i}"), str(tmp_path / f"twin{i}")
        assert sorted(os.listdir(mine)) == sorted(os.listdir(twin)) == ["12", "6", "best"], i
        for d in ("best", "6", "12"):
            assert sorted(os.listdir(os.path.join(mine, d))) == ["qnet.pt", "qnet_tgt.pt"]
            for f in ("qnet.pt", "qnet_tgt.pt"):
                assert open(os.path.join(mine, d, f), "rb").read() == open(os.path.join(twin, d, f), "rb").read(), (i, d, f)
            a, b = saved(B, i, os.path.join(mine, d)), saved(B, i, os.path.join(twin, d))
            for k in ("qnet", "qnet_tgt"):
                assert (bits(a[k]) == bits(b[k])).all(), (i, d, k)
    g.close()
    for rb in bufs: rb.close()


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_group_evaluate_equals_evaluator_on_twins(B, train):
    want, want_next = [], []
    fresh = np.random.default_rng(5).standard_normal((1, SHAPE[0])).astype(np.float32)
    for i in range(P):
        a = B.CandleDqn.build(online_config(B, i))
        a.train() if train else a.eval()
        want.append(evaluator(i).evaluate(a))
        act, info = a.sample(fresh, return_info=True)
        want_next.append((act.tolist(), info))
        a.close()
    g = B.CandleDqnGroup.build([online_config(B, i) for i in range(P)])
    for m in g.members: m.train() if train else m.eval()
    got = g.evaluate([evaluator(i) for i in range(P)])
    for i in range(P):
        same_result(got[i], want[i], i)
        assert got[i].n_episodes == N_EPISODES[i]
    assert got[1].normalized is not None and got[0].normalized is None
    assert len({r.n_steps for r in got}) == 3   # the members finished on different rounds: the subset launch was exercised
    for i, m in enumerate(g.members):           # the explorer streams and counters ended where the twins' did
        act, info = m.sample(fresh, return_info=True)
        assert (act.tolist(), info) == want_next[i], i
    g.close()
