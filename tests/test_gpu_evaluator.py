"""bdr_evaluate and the Trainer's post-processing (csrc/trainer.hip) with a real IQL agent on the GPU: a small deterministic
environment in Python behind the evaluator's callbacks, float64 observation rows and a normaliser, on both acting paths.

The expected score is a numpy replay of the reference's loop (default_evaluator.rs:64-88) whose actions come from `agent.sample` on
numpy-normalised rows: the acting paths are bit-equal (tests/test_gpu_dense_act.py), so the trajectories are identical and the
f32 score is compared with `==`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import iql_restatement as R  # noqa: E402

O, A = 11, 3
LENGTHS = (6, 5, 7)          # episode 1 ends by termination at its 5th step, the others by truncation


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


class AffineEnv:
    """state' = M state + G act + c (float64), reward = w . state' + v . act; the initial state depends on ix"""
    def __init__(self):
        rng = np.random.default_rng(3)
        q, _ = np.linalg.qr(rng.standard_normal((O, O)))
        self.M, self.G = 0.9 * q, 0.5 * rng.standard_normal((O, A))
        self.c, self.w, self.v = 0.1 * rng.standard_normal(O), rng.standard_normal(O), rng.standard_normal(A)
        self.base, self.dirs = 5.0 + rng.standard_normal(O), rng.standard_normal(O)
        self.calls = []

    def reset_with_index(self, ix):
        self.ix, self.t = ix, 0
        self.s = self.base + 0.25 * ix * self.dirs
        self.calls.append(("reset", ix))
        return self.s

    def step(self, act):
        act = np.asarray(act, np.float64)
        self.s = self.M @ self.s + self.G @ act + self.c
        self.t += 1
        r = float(self.w @ self.s + self.v @ act)
        term = self.ix == 1 and self.t == LENGTHS[1]
        trunc = self.ix != 1 and self.t == LENGTHS[self.ix]
        return self.s, r, term, trunc


def normaliser(B):
    k = np.arange(O)
    mean, std = (5.0 + 0.01 * k).astype(np.float32), (1.0 + 0.125 * (k % 4)).astype(np.float32)
    return B.ObsNormalizer(O, 0).set(mean, std), mean, std


def replay_score(agent, mean, std, n_episodes=3):
    """the reference's loop in numpy; the agent acts on numpy-normalised rows through its ordinary sample"""
    env, r_total, n_steps = AffineEnv(), np.float32(0), 0
    for ix in range(n_episodes):
        s = env.reset_with_index(ix)
        while True:
            z = ((s.astype(np.float32) - mean) / std).reshape(1, O)
            s, r, term, trunc = env.step(agent.sample(z)[0])
            r_total = np.float32(r_total + np.float32(r))
            n_steps += 1
            if term or trunc:
                break
    return np.float32(r_total / np.float32(n_episodes)), n_steps


SPEC = R.IqlSpec(O, A, (32, 32), (64, 64), (32, 32))


def agent(B, params, path="default", **kw):
    a = B.Iql.build(SPEC.to_config(B, 32, device=0, **kw))
    actor, critics, tgts, value = params
    a.set_params(actor, "actor"); a.set_params(value, "value")
    for i in range(SPEC.n_critics):
        a.set_params(critics[i], f"critic_{i}"); a.set_params(tgts[i], f"critic_tgt_{i}")
    a.set_act_path(path)
    return a


def buffer(B, seed=7):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=256, seed=seed), (O,), np.float32, (A,), np.float32)
    rb.push(*R.make_batch(SPEC, 200, 77))
    return rb


@pytest.mark.parametrize("path", ("layers", "fused"))
def test_evaluate_returns_the_f32_score_of_the_replayed_loop(B, path):
    params = SPEC.init_params(4)
    a = agent(B, params, path)
    a.eval()
    norm, mean, std = normaliser(B)
    env = AffineEnv()
    ev = B.Evaluator(env, 3, obs_norm=norm, obs_dtype=np.float64, act_dim=A, ref_scores=(-10.0, 30.0))
    res = ev.evaluate(a)
    want, n_steps = replay_score(a, mean, std)
    assert res.score == want, (res.score, want)
    assert (res.n_steps, res.n_episodes) == (n_steps, 3) == (sum(LENGTHS), 3)
    assert res.normalized == np.float32((want - np.float32(-10.0)) / (np.float32(30.0) - np.float32(-10.0)))
    assert env.calls == [("reset", 0), ("reset", 1), ("reset", 2)]
    # evaluation does not touch the mode: an agent in train mode is evaluated with its noise, and stays in train mode
    a.train()
    noisy = ev.evaluate(a)
    assert noisy.score != res.score and noisy.n_steps == n_steps
    on = C.c_int32()
    B._lib.check(B._lib.lib().bdr_agent_is_train(a.handle, C.byref(on)))
    assert on.value == 1
    a.close(); norm.close()


def test_train_offline_with_post_processing(B, tmp_path):
    params = SPEC.init_params(4)
    norm, mean, std = normaliser(B)
    a, twin, plain = agent(B, params, seed=5), agent(B, params, seed=5), agent(B, params, seed=5)
    rb, rb_twin, rb_plain = buffer(B), buffer(B), buffer(B)
    ev = B.Evaluator(AffineEnv(), 3, obs_norm=norm, obs_dtype=np.float64, act_dim=A)
    events = []
    model_dir = str(tmp_path / "model")
    tr = B.NativeTrainer(B.TrainerConfig(max_opts=6))
    st = tr.train_offline(a, rb, on_event=lambda e, o, kind, sc: events.append((o, kind, sc)), evaluator=ev, eval_interval=2, save_interval=3,
                          model_dir=model_dir)
    assert st["opt_steps"] == 6
    # the same steps by hand on a twin, evaluated after steps 2, 4 and 6
    want = []
    twin.train()
    for o in range(1, 7):
        twin.opt(rb_twin)
        if o % 2 == 0:
            twin.eval()
            want.append((o, [float(replay_score(twin, mean, std)[0])]))
            twin.train()
    got = [(o, sc) for o, kind, sc in events if kind == "eval"]
    assert got == want, (got, want)
    scores = [sc[0] for _, sc in want]
    # model_dir/best holds the model of the first strict maximum
    best = agent(B, SPEC.init_params(99))
    best.load_params(os.path.join(model_dir, "best"))
    best.eval()
    assert float(ev.evaluate(best).score) == max(scores)
    # model_dir/6 holds the final parameters bit for bit; model_dir/3 exists
    last = agent(B, SPEC.init_params(99))
    last.load_params(os.path.join(model_dir, "6"))
    for name in ("actor", "value", "critic_0", "critic_1"):
        assert (last.get_params(name).view(np.uint32) == a.get_params(name).view(np.uint32)).all(), name
        assert (a.get_params(name) == twin.get_params(name)).all(), name
    assert sorted(os.listdir(model_dir)) == ["3", "6", "best"]
    assert sorted(os.listdir(os.path.join(model_dir, "3"))) == ["actor.pt", "critic.pt", "critic.tgt.pt", "value.pt"]
    # after the run: train mode, and the noise stream where a run without evaluation leaves it (eval mode draws nothing)
    on = C.c_int32()
    B._lib.check(B._lib.lib().bdr_agent_is_train(a.handle, C.byref(on)))
    assert on.value == 1
    B.NativeTrainer(B.TrainerConfig(max_opts=6)).train_offline(plain, rb_plain)
    assert (a.draw_noise(16) == plain.draw_noise(16)).all()
    for x in (a, twin, plain, best, last, rb, rb_twin, rb_plain, norm):
        x.close()
