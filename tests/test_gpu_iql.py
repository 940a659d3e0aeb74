"""HIP IQL agent (csrc/iql.hip, through the C ABI) against the committed goldens and the float32 autograd restatement of
border-candle-agent's Iql::opt_ (tests/iql_restatement.py)."""
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
import iql_restatement as R  # noqa: E402
import make_golden_iql as MG  # noqa: E402


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def _agent(B, spec, bsz, params, **kw):
    a = B.Iql.build(spec.to_config(B, bsz, device=0, **kw))
    actor, critics, tgts, value = params
    a.set_params(actor, "actor"); a.set_params(value, "value")
    for i in range(spec.n_critics):
        a.set_params(critics[i], f"critic_{i}"); a.set_params(tgts[i], f"critic_tgt_{i}")
    return a


def _check_state(a, ref, spec, tag, lr_bar=0.3, tgt_bar=1e-5):
    """parameters within 0.3 lr, targets within 1e-5 relative (the bars of tests/test_gpu_sac.py:_run)"""
    assert np.abs(a.get_params("actor") - ref.params("actor")).max() < lr_bar * spec.lr_actor, tag
    assert np.abs(a.get_params("value") - ref.params("value")).max() < lr_bar * spec.lr_value, tag
    for i in range(spec.n_critics):
        assert np.abs(a.get_params(f"critic_{i}") - ref.params(f"critic_{i}")).max() < lr_bar * spec.lr_critic, (tag, i)
        assert rel(a.get_params(f"critic_tgt_{i}"), ref.params(f"critic_tgt_{i}")) < tgt_bar, (tag, i)


def _check_grads(a, pr, spec, tag):
    assert rel(a.get_params("value", "grad"), pr["value_grad"]) < 2e-3, (tag, rel(a.get_params("value", "grad"), pr["value_grad"]))
    assert rel(a.get_params("actor", "grad"), pr["actor_grad"]) < 2e-3, (tag, rel(a.get_params("actor", "grad"), pr["actor_grad"]))
    for i in range(spec.n_critics):
        assert rel(a.get_params(f"critic_{i}", "grad"), pr["critic_grads"][i]) < 2e-3, (tag, i)


def _check_rec(rec, r, tag):
    for k in ("loss_value", "loss_critic", "loss_actor"):
        assert abs(rec[k] - r[k]) <= 5e-4 * abs(r[k]) + 1e-6, (tag, k, rec[k], r[k])


def _check_probes(a, pr, bsz, tag):
    for k in ("q_tgt_min_value", "v", "tgt", "v_next", "q_tgt_min_actor", "v_obs", "logp"):
        assert rel(a.probe(k, bsz), pr[k]) < 1e-4, (tag, k, rel(a.probe(k, bsz), pr[k]))
    assert rel(a.probe("q_pred", bsz), pr["q_pred"]) < 1e-4, tag
    assert np.abs(a.probe("u", bsz) - pr["u"]).max() < 1e-4 * np.abs(pr["q_tgt_min_value"]).max() + 1e-6, tag
    assert rel(a.probe("w", bsz), pr["w"]) < 2e-3, tag


# ---------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_iql_goldens(B, golden_dir, name):
    spec, bsz, steps, seed = MG.case(name)
    g = np.load(os.path.join(golden_dir, f"iql_{name}.npz"))
    params = (g["actor0"], [g[f"critic{i}_0"] for i in range(spec.n_critics)], [g[f"critic{i}_0"] for i in range(spec.n_critics)], g["value0"])
    a = _agent(B, spec, bsz, params)
    for s in range(steps):
        batch = [g[f"s{s}_{k}"] for k in MG.BATCH_KEYS]
        rec = a.update_on_batch(*batch)
        for k in ("loss_value", "loss_critic", "loss_actor"):
            assert abs(rec[k] - g[f"s{s}_{k}"]) <= 5e-4 * abs(g[f"s{s}_{k}"]) + 1e-6, (name, s, k, rec[k], float(g[f"s{s}_{k}"]))
        for m, lr in (("actor", spec.lr_actor), ("value", spec.lr_value)):
            assert rel(a.get_params(m, "grad"), g[f"s{s}_{m}_grad"]) < 2e-3, (name, s, m)
            assert np.abs(a.get_params(m) - g[f"s{s}_{m}"]).max() < 0.3 * lr, (name, s, m)
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
    ref = R.IqlRestatement(spec, *params)
    for s in range(steps):
        batch = R.make_batch(spec, bsz, seed * 100 + s)
        rec = a.update_on_batch(*batch)
        r = ref.update(*batch)
        _check_rec(rec, r, (s,))
        _check_grads(a, ref.probes, spec, (s,))
        _check_probes(a, ref.probes, bsz, (s,))
        _check_state(a, ref, spec, (s,))
    assert a.n_opts == steps
    return a, ref


@pytest.mark.parametrize("steps", [1, 5])
def test_iql_pen_shape_against_the_restatement(B, steps):
    """examples/d4rl/iql_pen: obs 45, act 24, [256, 256, 256] for every net, B = 256; free-running updates, no re-seeding."""
    spec = R.IqlSpec(45, 24, (256, 256, 256), (256, 256, 256), (256, 256, 256))
    a, _ = _free_run(B, spec, 256, steps, 11)
    a.close()


@pytest.mark.parametrize("od,ad,units,nc,bsz,extra", [
    (17, 6, (64, 48), 1, 1, {}),
    (70, 5, (100,), 3, 7, {"critic_loss": "SmoothL1", "action_limit": "Tanh", "action_scale": 2.0}),
    (33, 13, (96, 80), 2, 300, {"adv_softmax": True, "v_relu_out": True, "q_relu_out": True}),
])
def test_iql_ragged_shapes(B, od, ad, units, nc, bsz, extra):
    spec = R.IqlSpec(od, ad, units, units[::-1], units, n_critics=nc, **extra)
    a, _ = _free_run(B, spec, bsz, 3, 5)
    a.close()


def test_iql_is_truncated_counts_in_gamma_not_done(B):
    spec = R.IqlSpec(9, 3, (32,), (32,), (32,))
    params = spec.init_params(2)
    a = _agent(B, spec, 8, params)
    obs, act, nxt, rew, _, _ = R.make_batch(spec, 8, 4)
    term, trunc = np.zeros(8, np.int8), np.ones(8, np.int8)
    a.update_on_batch(obs, act, nxt, rew, term, trunc)
    assert (a.probe("tgt", 8) == rew).all()           # gnd = 0: tgt = r exactly
    trunc[:] = 0
    a.update_on_batch(obs, act, nxt, rew, term, trunc)
    assert not (a.probe("tgt", 8) == rew).all()
    a.close()


def test_iql_two_agents_from_the_same_state_give_the_same_bits(B):
    spec = R.IqlSpec(45, 24, (256, 256), (256, 256), (256, 256), adv_softmax=True)
    params = spec.init_params(9)
    out = []
    for _ in range(2):
        a = _agent(B, spec, 300, params)
        recs = [a.update_on_batch(*R.make_batch(spec, 300, 40 + s)) for s in range(3)]
        out.append((recs, [a.get_params(m) for m in ("actor", "value", "critic_0", "critic_1", "critic_tgt_0")], a.probe("w", 300)))
        a.close()
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert (x == y).all()
    assert (out[0][2] == out[1][2]).all()


def _buffer(B, spec, n, seed):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=4096, seed=seed), (spec.obs_dim,), np.float32, (spec.act_dim,), np.float32)
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, n, 77)
    rb.push(obs, act, nxt, rew, term, trunc)
    return rb, (obs, act, nxt, rew, term, trunc)


def test_iql_opt_over_replay_with_three_updates_per_opt(B):
    """Agent::opt over the HBM ring, n_updates_per_opt = 3, against the restatement fed the indices of bdr_replay_sample_indices."""
    spec = R.IqlSpec(19, 4, (64, 64), (64, 64), (64, 64))
    params = spec.init_params(3)
    rb, rows = _buffer(B, spec, 1000, 42)
    twin, _ = _buffer(B, spec, 1000, 42)
    a = _agent(B, spec, 64, params, n_updates_per_opt=3)
    ref = R.IqlRestatement(spec, *params)
    for k in range(2):
        rec = a.opt_with_record(rb)
        rs = []
        for _ in range(3):
            ix = twin.sample_indices(64).astype(np.int64)
            rs.append(ref.update(*[x[ix] for x in rows]))
        for key in ("loss_value", "loss_critic", "loss_actor"):
            want = np.float32(sum(np.float32(r[key]) for r in rs)) / np.float32(3)
            assert abs(rec[key] - want) <= 5e-4 * abs(want) + 1e-6, (k, key, rec[key], want)
        _check_state(a, ref, spec, k)
    assert a.n_opts == 6
    a.close(); rb.close(); twin.close()


def test_iql_offline_trainer(B):
    """Trainer::train_offline (csrc/trainer.hip) runs N opts of an IQL agent; the observer's records are the restatement's."""
    spec = R.IqlSpec(12, 3, (32, 32), (32, 32), (32, 32))
    params = spec.init_params(8)
    rb, rows = _buffer(B, spec, 500, 7)
    twin, _ = _buffer(B, spec, 500, 7)
    a = _agent(B, spec, 32, params)
    events = []
    tr = B.NativeTrainer(B.TrainerConfig(max_opts=6, record_agent_info_interval=2))
    st = tr.train_offline(a, rb, on_event=lambda e, o, kind, sc: events.append((o, kind, sc)))
    assert st["opt_steps"] == 6 and a.n_opts == 6
    ref = R.IqlRestatement(spec, *params)
    recs = {}
    for o in range(1, 7):
        ix = twin.sample_indices(32).astype(np.int64)
        recs[o] = ref.update(*[x[ix] for x in rows])
    got = [(o, sc) for o, kind, sc in events if kind == "opt_record"]
    assert [o for o, _ in got] == [2, 4, 6]
    for o, sc in got:
        for v, key in zip(sc, ("loss_value", "loss_critic", "loss_actor")):
            assert abs(v - recs[o][key]) <= 5e-4 * abs(recs[o][key]) + 1e-6, (o, key, v, recs[o][key])
    _check_state(a, ref, spec, "offline")
    a.close(); rb.close(); twin.close()


@pytest.mark.parametrize("limit", ["Clamp", "Tanh"])
def test_iql_sample(B, limit):
    spec = R.IqlSpec(10, 4, (32,), (32, 32), (32,), action_limit=limit, action_scale=1.5, action_min=-0.3, action_max=0.4)
    params = spec.init_params(6)
    a = _agent(B, spec, 16, params, seed=21)
    ref = R.IqlRestatement(spec, *params)
    obs = np.random.default_rng(1).standard_normal((9, 10)).astype(np.float32)
    a.eval()
    e1, e2 = a.sample(obs), a.sample(obs)
    assert (e1 == e2).all()
    assert np.abs(e1 - ref.sample(obs)).max() < 1e-5
    a.train()
    t1 = a.sample(obs)
    b = _agent(B, spec, 16, params, seed=21)      # the same stream from the start: draw_noise replays what sample drew
    z = b.draw_noise(9 * 4).reshape(9, 4)
    assert np.abs(t1 - ref.sample(obs, z)).max() < 1e-5
    assert not np.allclose(t1, a.sample(obs))     # the stream advances
    a.close(); b.close()


def _safetensors_names(path):
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        hdr = json.loads(f.read(n))
    return {k: v["shape"] for k, v in hdr.items() if k != "__metadata__"}


def test_iql_checkpoint_files_names_and_the_critic_tgt_quirk(B, tmp_path):
    spec = R.IqlSpec(8, 3, (16, 16), (16,), (16, 16))
    params = spec.init_params(1)
    a = _agent(B, spec, 32, params)
    for s in range(2):
        a.update_on_batch(*R.make_batch(spec, 32, s))
    files = a.save_params(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["actor.pt", "critic.pt", "critic.tgt.pt", "value.pt"]
    names = _safetensors_names(files[0])
    assert names["actor.head2"] == [1, 3] and names["actor.mlp.ln0.weight"] == [16, 8] and names["actor.mlp.ln1.bias"] == [3]
    assert set(_safetensors_names(files[1])) == {f"critic{i}.mlp.ln{k}.{t}" for i in range(2) for k in range(3) for t in ("weight", "bias")}
    assert _safetensors_names(files[3])["value.mlp.ln2.weight"] == [1, 16]
    assert open(files[1], "rb").read() == open(files[2], "rb").read()   # critic.tgt.pt holds the ONLINE critics (util/critic.rs:272-285)
    b = B.Iql.build(spec.to_config(B, 32, device=0, seed=99))
    tgt_before = [b.get_params(f"critic_tgt_{i}") for i in range(2)]
    b.load_params(str(tmp_path))
    for m in ("actor", "value", "critic_0", "critic_1"):
        assert (b.get_params(m) == a.get_params(m)).all(), m
    for i in range(2):
        assert (b.get_params(f"critic_tgt_{i}") == tgt_before[i]).all()   # load leaves the targets alone
    a.close(); b.close()


def test_iql_rejects(B):
    spec = R.IqlSpec(8, 3, (16,), (16,), (16,))
    cfg = spec.to_config(B, 4, device=0)
    cfg.value_config = B.ValueConfig(B.CandleMlpConfig((16,), "Tanh"))       # activation_out Tanh / Sigmoid: not supported
    with pytest.raises(B.BdrError):
        B.Iql.build(cfg)
    cfg = spec.to_config(B, 4, device=0)
    cfg.critic_config.opt_config = B.OptimizerConfig.AdamW(1e-3, amsgrad=True)   # candle's AdamW has no amsgrad
    with pytest.raises(B.BdrError):
        B.Iql.build(cfg)
