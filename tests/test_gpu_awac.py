"""HIP AWAC agent (csrc/awac.hip, through the C ABI) against the committed goldens and the float32 autograd restatement of
border-candle-agent's Awac::opt_ (tests/awac_restatement.py).  Tolerances are those of tests/test_gpu_iql.py."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import awac_restatement as R  # noqa: E402
import iql_restatement as RI  # noqa: E402
import make_golden_awac as MG  # noqa: E402


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def _agent(B, spec, bsz, params, train=True, **kw):
    a = B.Awac.build(spec.to_config(B, bsz, device=0, train=train, **kw))
    actor, critics, tgts = params
    a.set_params(actor, "actor")
    for i in range(spec.n_critics):
        a.set_params(critics[i], f"critic_{i}"); a.set_params(tgts[i], f"critic_tgt_{i}")
    return a


def _check_state(a, ref, spec, tag, lr_bar=0.3, tgt_bar=1e-5):
    """parameters within 0.3 lr, targets within 1e-5 relative (the bars of tests/test_gpu_iql.py)"""
    assert np.abs(a.get_params("actor") - ref.params("actor")).max() < lr_bar * spec.lr_actor, tag
    for i in range(spec.n_critics):
        assert np.abs(a.get_params(f"critic_{i}") - ref.params(f"critic_{i}")).max() < lr_bar * spec.lr_critic, (tag, i)
        assert rel(a.get_params(f"critic_tgt_{i}"), ref.params(f"critic_tgt_{i}")) < tgt_bar, (tag, i)


def _check_grads(a, pr, spec, tag):
    assert rel(a.get_params("actor", "grad"), pr["actor_grad"]) < 2e-3, (tag, rel(a.get_params("actor", "grad"), pr["actor_grad"]))
    for i in range(spec.n_critics):
        assert rel(a.get_params(f"critic_{i}", "grad"), pr["critic_grads"][i]) < 2e-3, (tag, i)


def _close(x, want, tag):
    assert abs(x - want) <= 5e-4 * abs(want) + 1e-6, (tag, x, want)


def _check_rec(rec, r, tag):
    for k in R.RECORD_KEYS:
        if k in ("adv_mean", "adv_abs_mean"):   # a mean of differences: bounded by the scale of the Q values
            assert abs(rec[k] - r[k]) <= 1e-4 * max(1.0, r["q_tgt_abs_mean"]) + 5e-4 * abs(r[k]), (tag, k, rec[k], r[k])
        else:
            _close(rec[k], r[k], (tag, k))


def _check_probes(a, pr, bsz, tag):
    for k in ("q_data_min", "q_pi_min", "next_q", "tgt", "logp", "act_", "next_act"):
        assert rel(a.probe(k, bsz), pr[k]) < 1e-4, (tag, k, rel(a.probe(k, bsz), pr[k]))
    assert rel(a.probe("q_pred", bsz), pr["q_pred"]) < 1e-4, tag
    assert np.abs(a.probe("adv", bsz) - pr["adv"]).max() < 1e-4 * np.abs(pr["q_data_min"]).max() + 1e-6, tag
    assert rel(a.probe("w", bsz), pr["w"]) < 2e-3, tag


# ---------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_awac_goldens(B, golden_dir, name):
    spec, bsz, steps, seed = MG.case(name)
    g = np.load(os.path.join(golden_dir, f"awac_{name}.npz"))
    crit = [g[f"critic{i}_0"] for i in range(spec.n_critics)]
    a = _agent(B, spec, bsz, (g["actor0"], crit, crit))
    for s in range(steps):
        batch = [g[f"s{s}_{k}"] for k in MG.BATCH_KEYS]
        rec = a.update_on_batch(*batch, g[f"s{s}_z_pi"], g[f"s{s}_z_next"])
        for k in ("loss_critic", "loss_actor", "q_tgt_abs_mean", "logp_mean", "reward_mean", "next_q_mean"):
            _close(rec[k], float(g[f"s{s}_{k}"]), (name, s, k))
        assert rel(a.get_params("actor", "grad"), g[f"s{s}_actor_grad"]) < 2e-3, (name, s)
        assert np.abs(a.get_params("actor") - g[f"s{s}_actor"]).max() < 0.3 * spec.lr_actor, (name, s)
        for i in range(spec.n_critics):
            assert rel(a.get_params(f"critic_{i}", "grad"), g[f"s{s}_critic{i}_grad"]) < 2e-3, (name, s, i)
            assert np.abs(a.get_params(f"critic_{i}") - g[f"s{s}_critic{i}"]).max() < 0.3 * spec.lr_critic, (name, s, i)
            assert rel(a.get_params(f"critic_tgt_{i}"), g[f"s{s}_critic_tgt{i}"]) < 1e-5, (name, s, i)
    assert a.n_opts == steps
    a.close()


# ---------------------------------------------------------------------------------------------------------- restatement
def _free_run(B, spec, bsz, steps, seed, **kw):
    params = spec.init_params(seed)
    a = _agent(B, spec, bsz, params, **kw)
    ref = R.AwacRestatement(spec, *params)
    for s in range(steps):
        batch = R.make_batch(spec, bsz, seed * 100 + s)
        z = spec.draws(bsz, seed * 100 + 50 + s)
        rec = a.update_on_batch(*batch, *z)
        r = ref.update(*batch, *z)
        _check_rec(rec, r, (s,))
        _check_grads(a, ref.probes, spec, (s,))
        _check_probes(a, ref.probes, bsz, (s,))
        _check_state(a, ref, spec, (s,))
    assert a.n_opts == steps
    return a, ref


@pytest.mark.parametrize("steps", [1, 5])
def test_awac_pen_shape_against_the_restatement(B, steps):
    """examples/d4rl/awac_pen: obs 45, act 24, [256, 256, 256] for actor and twin critics, B = 256; free-running updates."""
    spec = R.AwacSpec(45, 24, (256, 256, 256), (256, 256, 256))
    a, _ = _free_run(B, spec, 256, steps, 11)
    a.close()


# 1500 rows: two free-running steps.  The f32 drift between the two free runs (each parameter within 0.3 lr) grows with the row
# count; at the third step one critic's gradient was 3e-3 off (max-relative) while the 8 record values still agreed, which points
# at hidden ReLUs whose pre-activation crossed 0 rather than at a wrong sum.
@pytest.mark.parametrize("od,ad,units,nc,bsz,steps,extra", [
    (17, 6, (64, 48), 1, 7, 3, {"q_relu_out": True}),
    (70, 5, (100,), 3, 300, 3, {"critic_loss": "SmoothL1", "action_limit": "Tanh", "action_scale": 2.0}),
    (33, 13, (96, 80), 4, 1500, 2, {"adv_softmax": True}),
    (3, 1, (64, 64), 2, 45, 3, {"action_limit": "Tanh", "action_scale": 2.0}),   # examples/gym/awac_pendulum: A = 1
])
def test_awac_ragged_shapes(B, od, ad, units, nc, bsz, steps, extra):
    spec = R.AwacSpec(od, ad, units, units[::-1], n_critics=nc, **extra)
    a, _ = _free_run(B, spec, bsz, steps, 5)
    a.close()


def test_awac_rejects_a_one_row_batch(B):
    spec = R.AwacSpec(4, 2, (16,), (16,))
    with pytest.raises(B.BdrError, match="at least 2 rows"):
        B.Awac.build(spec.to_config(B, 1, device=0))
    a = _agent(B, spec, 8, spec.init_params(1))
    with pytest.raises(B.BdrError, match="at least 2 rows"):
        a.update_on_batch(*R.make_batch(spec, 1, 2))
    assert a.n_opts == 0
    a.close()


def test_awac_is_truncated_counts_in_gamma_not_done(B):
    spec = R.AwacSpec(9, 3, (32,), (32,))
    a = _agent(B, spec, 8, spec.init_params(2))
    obs, act, nxt, rew, _, _ = R.make_batch(spec, 8, 4)
    term, trunc = np.zeros(8, np.int8), np.ones(8, np.int8)
    a.update_on_batch(obs, act, nxt, rew, term, trunc)
    assert (a.probe("tgt", 8) == rew).all()           # gnd = 0: tgt = r exactly
    trunc[:] = 0
    a.update_on_batch(obs, act, nxt, rew, term, trunc)
    assert not (a.probe("tgt", 8) == rew).all()
    a.close()


def _state(a, nc):
    return [a.get_params(m) for m in ["actor"] + [f"critic_{i}" for i in range(nc)] + [f"critic_tgt_{i}" for i in range(nc)]]


def test_awac_two_agents_from_the_same_state_give_the_same_bits(B):
    spec = R.AwacSpec(45, 24, (256, 256), (256, 256), adv_softmax=True)
    params = spec.init_params(9)
    out = []
    for _ in range(2):
        a = _agent(B, spec, 300, params, seed=5)     # device noise: the same seeded stream
        recs = [a.update_on_batch(*R.make_batch(spec, 300, 40 + s)) for s in range(3)]
        out.append((recs, _state(a, 2), a.probe("w", 300), a.probe("next_act", 300)))
        a.close()
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert (x == y).all()
    assert (out[0][2] == out[1][2]).all() and (out[0][3] == out[1][3]).all()


def test_awac_device_noise_equals_the_same_draws_given_by_the_host(B):
    """NULL z: B*A draws for act_, then B*A for next_act, from the stream bdr_agent_draw_noise reads."""
    spec = R.AwacSpec(12, 4, (64, 64), (64, 64))
    params = spec.init_params(4)
    bsz = 40
    a = _agent(B, spec, bsz, params, seed=17)
    b = _agent(B, spec, bsz, params, seed=17)
    twin = _agent(B, spec, bsz, params, seed=17)
    for s in range(2):
        batch = R.make_batch(spec, bsz, 60 + s)
        z = twin.draw_noise(2 * bsz * spec.act_dim).reshape(2, bsz, spec.act_dim)
        ra = a.update_on_batch(*batch)
        rb = b.update_on_batch(*batch, z[0], z[1])
        assert ra == rb, s
        for x, y in zip(_state(a, 2), _state(b, 2)):
            assert (x == y).all(), s
    # host draws take nothing from b's stream; a's stream moved on by 2 updates x 2 B A
    fresh = _agent(B, spec, bsz, params, seed=17)
    assert (b.draw_noise(16) == fresh.draw_noise(16)).all()
    assert (a.draw_noise(16) == twin.draw_noise(16)).all()
    for x in (a, b, twin, fresh):
        x.close()


def test_awac_eval_mode_update_uses_the_means_and_no_draws(B):
    spec = R.AwacSpec(10, 3, (32, 32), (32, 32), action_min=-0.4, action_max=0.5)
    params = spec.init_params(6)
    a = _agent(B, spec, 24, params, train=False, seed=3)
    ref = R.AwacRestatement(spec, *params)
    batch = R.make_batch(spec, 24, 7)
    rec = a.update_on_batch(*batch)
    r = ref.update(*batch)     # z = None: the means
    _check_rec(rec, r, "eval")
    _check_probes(a, ref.probes, 24, "eval")
    fresh = _agent(B, spec, 24, params, seed=3)
    assert (a.draw_noise(32) == fresh.draw_noise(32)).all()   # no draws taken
    a.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------- replay, trainers
def _buffer(B, spec, n, seed, capacity=4096):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed), (spec.obs_dim,), np.float32, (spec.act_dim,), np.float32)
    rows = R.make_batch(spec, n, 77)
    rb.push(*rows)
    return rb, rows


def _replay_draws(twin, bsz, A):
    z = twin.draw_noise(2 * bsz * A).reshape(2, bsz, A)
    return z[0], z[1]


def test_awac_opt_over_replay_with_three_updates_per_opt(B):
    """Agent::opt over the HBM ring, n_updates_per_opt = 3, train mode on the device stream, against the restatement fed the indices
    of bdr_replay_sample_indices and the draws of a same-seed twin; the 8-key record with its sum-versus-mean quirk."""
    spec = R.AwacSpec(19, 4, (64, 64), (64, 64))
    params = spec.init_params(3)
    rb, rows = _buffer(B, spec, 1000, 42)
    twin_rb, _ = _buffer(B, spec, 1000, 42)
    a = _agent(B, spec, 64, params, n_updates_per_opt=3, seed=8)
    twin = _agent(B, spec, 64, params, seed=8)
    ref = R.AwacRestatement(spec, *params)
    for k in range(2):
        rec = a.opt_with_record(rb)
        assert list(rec) == list(R.RECORD_KEYS)
        rs = []
        for _ in range(3):
            ix = twin_rb.sample_indices(64).astype(np.int64)
            rs.append(ref.update(*[x[ix] for x in rows], *_replay_draws(twin, 64, spec.act_dim)))
        _check_rec(rec, ref.opt_record(rs), k)
        _check_state(a, ref, spec, k)
    assert a.n_opts == 6
    a.close(); twin.close(); rb.close(); twin_rb.close()


def test_awac_offline_trainer(B):
    """Trainer::train_offline (csrc/trainer.hip) runs N opts of an AWAC agent; the observer's records are the restatement's."""
    spec = R.AwacSpec(12, 3, (32, 32), (32, 32))
    params = spec.init_params(8)
    rb, rows = _buffer(B, spec, 500, 7)
    twin_rb, _ = _buffer(B, spec, 500, 7)
    a = _agent(B, spec, 32, params, seed=2)
    twin = _agent(B, spec, 32, params, seed=2)
    events = []
    tr = B.NativeTrainer(B.TrainerConfig(max_opts=6, record_agent_info_interval=2))
    st = tr.train_offline(a, rb, on_event=lambda e, o, kind, sc: events.append((o, kind, sc)))
    assert st["opt_steps"] == 6 and a.n_opts == 6
    ref = R.AwacRestatement(spec, *params)
    recs = {}
    for o in range(1, 7):
        ix = twin_rb.sample_indices(32).astype(np.int64)
        recs[o] = ref.update(*[x[ix] for x in rows], *_replay_draws(twin, 32, spec.act_dim))
    got = [(o, sc) for o, kind, sc in events if kind == "opt_record"]
    assert [o for o, _ in got] == [2, 4, 6]
    for o, sc in got:
        assert len(sc) == 8
        _check_rec(dict(zip(R.RECORD_KEYS, sc)), recs[o], o)
    _check_state(a, ref, spec, "offline")
    a.close(); twin.close(); rb.close(); twin_rb.close()


def test_awac_online_trainer_with_a_float_action_env(B):
    """bdr_trainer_train with an AWAC handle (examples/gym/awac_pendulum's loop): the default function table samples f32 action
    rows (bdr_awac_sample) and pushes them through the generic act rows; the loop rules are the DQN ones."""
    od, ad = 3, 1
    spec = R.AwacSpec(od, ad, (64, 64), (64, 64), action_limit="Tanh", action_scale=2.0)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=200, seed=9), (od,), np.float32, (ad,), np.float32)
    a = _agent(B, spec, 16, spec.init_params(1), seed=3)
    env = B.SyntheticEnv((od,), np.float32, seed=11, p_term=0.1)
    ev = []
    st = B.NativeTrainer(B.TrainerConfig(max_opts=20, opt_interval=2, warmup_period=24, record_agent_info_interval=5)).train(
        env, a, rb, (od,), np.float32, act_row_bytes=ad * 4, act_dtype=np.float32, on_event=lambda e, o, k, sc: ev.append((e, o, k, sc)))
    a.sync()
    assert st["opt_steps"] == a.n_opts == 20 and st["env_steps"] == rb.len() and 24 + 2 * 19 <= st["env_steps"] <= 24 + 2 * 20
    recs = [sc for _, _, k, sc in ev if k == "opt_record"]
    assert len(recs) == 4 and all(len(sc) == 8 and np.isfinite(sc).all() for sc in recs)
    b = rb.batch(32)
    assert b.act.dtype == np.float32 and (np.abs(b.act) <= 2.0).all() and np.abs(b.act).max() > 0
    assert len(np.unique(b.act)) > 8   # sampled actions, not one constant
    a.close(); rb.close()


def test_awac_async_actors_sample_awac_actions(B):
    """the compiled async loops with AWAC handles: actors sample f32 actions (bdr_actor_ops_default dispatches Policy::sample by
    agent kind) and adopt the learner's actor through the device mailbox; critics stay the actors' own."""
    od, ad, n_act, max_opts, warm = 5, 2, 2, 20, 96
    spec = R.AwacSpec(od, ad, (64, 64), (64, 64), action_min=-0.5, action_max=0.5)
    learner = _agent(B, spec, 32, spec.init_params(1), seed=1)
    actors = [_agent(B, spec, 32, spec.init_params(10 + i), seed=10 + i) for i in range(n_act)]
    q_before = [x.get_params("critic_0").copy() for x in actors]
    envs = [B.SyntheticEnv((od,), np.float32, seed=i, p_term=0.1) for i in range(n_act)]
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=500, seed=42), (od,), np.float32, (ad,), np.float32)
    events = []
    tr = B.AsyncTrainer(B.AsyncTrainerConfig(max_opts=max_opts, warmup_period=warm, sync_interval=5, record_agent_info_interval=10,
                                             record_compute_cost_interval=0, warmup_sleep_ms=5), B.ActorManagerConfig(n_buffer=16))
    st = tr.train(learner, rb, actors, envs, (od,), np.float32, act_row_bytes=ad * 4, act_dtype=np.float32, on_event=lambda *e: events.append(e))
    assert st.opt_steps == max_opts and learner.n_opts == max_opts
    recs = [e for e in events if e[3] == "opt_record"]
    assert len(recs) == max_opts // 10 and all(len(e[4]) == 8 and np.isfinite(e[4]).all() for e in recs)
    b = rb.batch(64)
    assert b.act.dtype == np.float32 and b.act.shape == (64, ad) and (np.abs(b.act) <= 0.5).all() and np.abs(b.act).max() > 0
    synced = {e[0]: e[2] for e in events if e[3] == "actor_sync"}
    for i, x in enumerate(actors):
        assert (x.get_params("critic_0") == q_before[i]).all()
        if synced.get(i) == max_opts:
            assert (x.get_params("actor") == learner.get_params("actor")).all()
    assert any(v > 0 for v in synced.values())
    for x in actors:
        x.close()
    learner.close(); rb.close()


# ---------------------------------------------------------------------------------------------------------- sample, checkpoints, rejects
@pytest.mark.parametrize("limit", ["Clamp", "Tanh"])
def test_awac_sample(B, limit):
    spec = R.AwacSpec(10, 4, (32, 32), (32,), action_limit=limit, action_scale=1.5, action_min=-0.3, action_max=0.4)
    params = spec.init_params(6)
    a = _agent(B, spec, 16, params, train=False, seed=21)
    ref = R.AwacRestatement(spec, *params)
    obs = np.random.default_rng(1).standard_normal((9, 10)).astype(np.float32)
    e1, e2 = a.sample(obs), a.sample(obs)
    assert (e1 == e2).all()
    assert np.abs(e1 - ref.sample(obs).numpy()).max() < 1e-5
    a.train()
    t1 = a.sample(obs)
    b = _agent(B, spec, 16, params, seed=21)      # the same stream from the start: draw_noise replays what sample drew
    z = b.draw_noise(9 * 4).reshape(9, 4)
    assert np.abs(t1 - ref.sample(obs, z).numpy()).max() < 1e-5
    assert not np.allclose(t1, a.sample(obs))     # the stream advances
    a.close(); b.close()


def _safetensors_names(path):
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        hdr = json.loads(f.read(n))
    return {k: v["shape"] for k, v in hdr.items() if k != "__metadata__"}


def test_awac_checkpoint_files_names_and_the_critic_tgt_quirk(B, tmp_path):
    spec = R.AwacSpec(8, 3, (16,), (16, 16))
    a = _agent(B, spec, 32, spec.init_params(1))
    for s in range(2):
        a.update_on_batch(*R.make_batch(spec, 32, s))
    files = a.save_params(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["actor.pt", "critic.pt", "critic.tgt.pt"]
    assert sorted(os.listdir(tmp_path)) == ["actor.pt", "critic.pt", "critic.tgt.pt"]
    names = _safetensors_names(files[0])
    assert names["actor.head2"] == [1, 3] and names["actor.mlp.ln0.weight"] == [16, 8] and names["actor.mlp.ln1.bias"] == [3]
    assert set(_safetensors_names(files[1])) == {f"critic{i}.mlp.ln{k}.{t}" for i in range(2) for k in range(3) for t in ("weight", "bias")}
    assert open(files[1], "rb").read() == open(files[2], "rb").read()   # critic.tgt.pt holds the ONLINE critics (util/critic.rs:272-285)
    b = B.Awac.build(spec.to_config(B, 32, device=0, seed=99))
    tgt_before = [b.get_params(f"critic_tgt_{i}") for i in range(2)]
    b.load_params(str(tmp_path))
    for m in ("actor", "critic_0", "critic_1"):
        assert (b.get_params(m) == a.get_params(m)).all(), m
    for i in range(2):
        assert (b.get_params(f"critic_tgt_{i}") == tgt_before[i]).all()   # load leaves the targets alone
    a.close(); b.close()


def test_awac_loads_what_iql_saved(B, tmp_path):
    """the same GaussianActor and MultiCritic VarMaps: IQL's actor.pt / critic.pt / critic.tgt.pt load into AWAC bit for bit"""
    ispec = RI.IqlSpec(8, 3, (16, 16), (16,), (16, 16))
    q = B.Iql.build(ispec.to_config(B, 16, device=0, seed=4))
    q.update_on_batch(*RI.make_batch(ispec, 16, 1))
    q.save_params(str(tmp_path))
    spec = R.AwacSpec(8, 3, (16,), (16, 16))
    a = B.Awac.build(spec.to_config(B, 16, device=0, seed=5))
    a.load_params(str(tmp_path))
    for m in ("actor", "critic_0", "critic_1"):
        assert (a.get_params(m) == q.get_params(m)).all(), m
    q.close(); a.close()


def test_awac_rejects(B):
    spec = R.AwacSpec(8, 3, (16,), (16,))
    for act in ("Tanh", "Sigmoid"):   # activation_out Tanh / Sigmoid: not supported
        cfg = spec.to_config(B, 4, device=0)
        cfg.critic_config.q_config = B.CandleMlpConfig((16,), act)
        with pytest.raises(B.BdrError):
            B.Awac.build(cfg)
    cfg = spec.to_config(B, 4, device=0)
    cfg.critic_config.opt_config = B.OptimizerConfig.AdamW(1e-3, amsgrad=True)   # candle's AdamW has no amsgrad
    with pytest.raises(B.BdrError):
        B.Awac.build(cfg)
    cfg = spec.to_config(B, 4, device=0)
    cfg.actor_config.opt_config = B.OptimizerConfig.AdamW(1e-3, amsgrad=True)
    with pytest.raises(B.BdrError):
        B.Awac.build(cfg)
    # synchronous data-parallel gradients: refused for an AWAC handle
    L = B._lib.lib()
    uid = (C.c_uint8 * B._lib.BDR_UNIQUE_ID_BYTES)()
    B._lib.check(L.bdr_comm_get_unique_id(uid))
    h = C.c_void_p()
    B._lib.check(L.bdr_comm_init_rank(uid, 1, 0, 0, C.byref(h)))
    a = B.Awac.build(spec.to_config(B, 4, device=0))
    assert L.bdr_agent_set_grad_comm(a.handle, h) == 1   # BDR_ERR_INVALID
    assert b"AWAC" in L.bdr_last_error()
    a.close()
    B._lib.check(L.bdr_comm_destroy(h))
