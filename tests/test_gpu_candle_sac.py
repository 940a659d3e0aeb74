"""HIP candle SAC agent (csrc/candle_sac.hip, through the C ABI) against the committed goldens and the float32 autograd restatement
of border-candle-agent's Sac::opt_ (tests/candle_sac_restatement.py).

Bars are those of tests/test_gpu_awac.py - parameters within 0.3 lr, gradients 2e-3 max-relative, probes 1e-4, targets 1e-5 - and,
wherever float32 arithmetic alone moves the restatement further, 4 x the float32-versus-float64 figure of the same restatement on
the same inputs (R.f32_f64_figures; tests/test_candle_sac_restatement.py prints them per case).  That happens with the Tanh limit:
the log-Jacobian clamps the action itself at 0.999999, whose float32 neighbour 0.99999899 moves ln(1 - a^2) by 1.3e-2 per clamped
element, and the atanh round trip loses bits as |a / scale| approaches 1.  Draws are scaled (R.CandleSacSpec.draws) so that on
every row |a / scale| < 0.999: saturation is tests/test_gpu_candle_sac_edges.py's subject."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import candle_sac_restatement as R  # noqa: E402
import make_golden_candle_sac as MG  # noqa: E402

rel = R.rel
Z = 0.4   # the draws' spread


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _agent(B, spec, bsz, params, train=True, **kw):
    a = B.CandleSac.build(spec.to_config(B, bsz, device=0, train=train, **kw))
    actor, critics, tgts = params
    a.set_params(actor, "actor")
    for i in range(spec.n_critics):
        a.set_params(critics[i], f"critic_{i}"); a.set_params(tgts[i], f"critic_tgt_{i}")
    return a


def bar(base, fig):
    """the AWAC bar, or 4 x the restatement's own float32-versus-float64 figure where that is larger"""
    return max(base, 4.0 * float(fig))


def _close(x, want, tag, tol=5e-4):
    assert abs(x - want) <= tol * abs(want) + 1e-6, (tag, x, want)


def _check_step(a, spec, bsz, want, fig, tag):
    """want: name -> the float32 restatement's value (probes, gradients, parameters); fig: its f32-vs-f64 figures"""
    for k in ("a", "logp", "q_min", "dq_da", "next_a", "next_logp", "tgt"):
        got = a.probe(k, bsz)
        print(tag, k, rel(got, want[k]), "bar", bar(1e-4, fig[k]))
        assert rel(got, want[k]) < bar(1e-4, fig[k]), (tag, k, rel(got, want[k]), fig[k])          # probes 1e-4, or 4 x fig
    if "q_pred" in want:
        assert rel(a.probe("q_pred", bsz), want["q_pred"]) < bar(1e-4, fig["q_pred"]), tag
    g = a.get_params("actor", "grad")
    print(tag, "actor_grad", rel(g, want["actor_grad"]), "bar", bar(2e-3, fig["actor_grad"]))
    assert rel(g, want["actor_grad"]) < bar(2e-3, fig["actor_grad"]), (tag, rel(g, want["actor_grad"]))   # gradients 2e-3, or 4 x fig
    assert np.abs(a.get_params("actor") - want["actor"]).max() < bar(0.3 * spec.lr_actor, fig["actor"]), tag   # 0.3 lr, or 4 x fig
    for i in range(spec.n_critics):
        gi = a.get_params(f"critic_{i}", "grad")
        assert rel(gi, want["critic_grads"][i]) < bar(2e-3, fig["critic_grad"]), (tag, i, rel(gi, want["critic_grads"][i]))
        assert np.abs(a.get_params(f"critic_{i}") - want["critics"][i]).max() < bar(0.3 * spec.lr_critic, fig["critic"]), (tag, i)
        assert rel(a.get_params(f"critic_tgt_{i}"), want["critic_tgts"][i]) < 1e-5, (tag, i)       # targets 1e-5
    if spec.ent_coef[0] == "Auto":
        assert abs(float(a.get_params("log_alpha")[0]) - float(want["log_alpha"][0])) < 0.3 * spec.ent_coef[2], tag


# ---------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_candle_sac_goldens(B, golden_dir, name):
    spec, bsz, steps, seed = MG.case(name)
    g = np.load(os.path.join(golden_dir, f"candle_sac_{name}.npz"))
    crit = [g[f"critic{i}_0"] for i in range(spec.n_critics)]
    a = _agent(B, spec, bsz, (g["actor0"], crit, crit))
    for s in range(steps):
        batch = [g[f"s{s}_{k}"] for k in MG.BATCH_KEYS]
        rec = a.update_on_batch(*batch, g[f"s{s}_z_pi"], g[f"s{s}_z_next"])
        fig = {k: float(g[f"s{s}_fig_{k}"]) for k in R.FIGURE_KEYS}
        _close(rec["loss_critic"], float(g[f"s{s}_loss_critic"]), (name, s, "loss_critic"), bar(5e-4, 2 * fig["tgt"]))
        _close(rec["loss_actor"], float(g[f"s{s}_loss_actor"]), (name, s, "loss_actor"), bar(5e-4, fig["logp"]))
        _close(rec["ent_coef"], float(g[f"s{s}_ent_coef"]), (name, s, "ent_coef"))
        want = {k: g[f"s{s}_{k}"] for k in MG.PROBE_KEYS}
        want.update(actor_grad=g[f"s{s}_actor_grad"], actor=g[f"s{s}_actor"], log_alpha=g[f"s{s}_log_alpha"],
                    critic_grads=[g[f"s{s}_critic{i}_grad"] for i in range(spec.n_critics)],
                    critics=[g[f"s{s}_critic{i}"] for i in range(spec.n_critics)],
                    critic_tgts=[g[f"s{s}_critic_tgt{i}"] for i in range(spec.n_critics)])
        _check_step(a, spec, bsz, want, fig, (name, s))
    assert a.n_opts == steps
    a.close()


# ---------------------------------------------------------------------------------------------------------- restatement
def _want(ref, spec):
    w = dict(ref.probes)
    w.update(actor=ref.params("actor"), log_alpha=ref.params("log_alpha"),
             critics=[ref.params(f"critic_{i}") for i in range(spec.n_critics)],
             critic_tgts=[ref.params(f"critic_tgt_{i}") for i in range(spec.n_critics)])
    return w


def _free_run(B, spec, bsz, steps, seed, z_scale=Z, **kw):
    params = spec.init_params(seed)
    a = _agent(B, spec, bsz, params, **kw)
    ref = R.CandleSacRestatement(spec, *params)
    ref64 = R.CandleSacRestatement(spec, *params, dtype=torch.float64)
    for s in range(steps):
        batch = R.make_batch(spec, bsz, seed * 100 + s)
        z = spec.draws(bsz, seed * 100 + 50 + s, z_scale)
        rec = a.update_on_batch(*batch, *z)
        r = ref.update(*batch, *z)
        ref64.update(*batch, *z)
        fig = R.f32_f64_figures(ref, ref64)
        if spec.action_limit == "Tanh":
            assert max(np.abs(ref.probes[k] / spec.action_scale).max() for k in ("a", "next_a")) < 0.999, "the case must stay off saturation"
        _close(rec["loss_critic"], r["loss_critic"], (s, "loss_critic"), bar(5e-4, 2 * fig["tgt"]))
        _close(rec["loss_actor"], r["loss_actor"], (s, "loss_actor"), bar(5e-4, fig["logp"]))
        _close(rec["ent_coef"], r["ent_coef"], (s, "ent_coef"))
        _check_step(a, spec, bsz, _want(ref, spec), fig, (s,))
    assert a.n_opts == steps
    return a, ref


@pytest.mark.parametrize("kind,limit", [("Mlp2", "Tanh"), ("Mlp2", "Clamp"), ("Mlp3", "Tanh")])
def test_candle_sac_pendulum_shape_against_the_restatement(B, kind, limit):
    """examples/gym/sac_pendulum: obs 3, act 1, [64, 64] for the Mlp2 actor and the twin critics, Tanh{2}, Auto; B = 32 here"""
    spec = R.CandleSacSpec(3, 1, (64, 64), (64, 64), actor_kind=kind, action_limit=limit, action_scale=2.0, ent_coef=("Auto", -1.0, 3e-4))
    a, _ = _free_run(B, spec, 32, 3, 7)
    a.close()


@pytest.mark.parametrize("od,ad,units,nc,bsz,steps,extra", [
    # three critics, an odd batch over one 32-row block, widths that are no multiple of the 32 / 64 tiles
    (5, 3, (24, 40), 3, 37, 3, {"actor_kind": "Mlp2", "action_limit": "Tanh", "action_scale": 1.5, "ent_coef": ("Auto", -3.0, 1e-3), "critic_loss": "SmoothL1"}),
    (5, 3, (24, 40), 3, 37, 2, {"actor_kind": "Mlp3", "q_relu_out": True, "ent_coef": ("Fix", 0.3)}),
    # act 33 > 32: 2 A = 66 head columns pad to 128, a second 32-column tile; the smallest batch the reference can run
    (9, 33, (48, 32), 2, 2, 2, {"actor_kind": "Mlp2", "ent_coef": ("Auto", -33.0, 1e-3)}),
    (9, 33, (48, 32), 2, 2, 2, {"actor_kind": "Mlp3", "action_limit": "Tanh", "ent_coef": ("Fix", 0.1)}),
])
def test_candle_sac_ragged_shapes(B, od, ad, units, nc, bsz, steps, extra):
    spec = R.CandleSacSpec(od, ad, units, units[::-1], n_critics=nc, **extra)
    a, _ = _free_run(B, spec, bsz, steps, 5)
    a.close()


def test_candle_sac_pen_shape_two_steps(B):
    """obs 45, act 24, [256, 256] for the Mlp2 actor and the twin critics, B = 256: the dW kernels' 256-row chunk"""
    spec = R.CandleSacSpec(45, 24, (256, 256), (256, 256), actor_kind="Mlp2", action_limit="Tanh", ent_coef=("Auto", -24.0, 3e-4))
    a, _ = _free_run(B, spec, 256, 2, 11, z_scale=0.3)
    a.close()


# ---------------------------------------------------------------------------------------------------------- noise, modes
def _state(a, nc):
    return [a.get_params(m) for m in ["actor", "log_alpha"] + [f"critic_{i}" for i in range(nc)] + [f"critic_tgt_{i}" for i in range(nc)]]


SMALL = dict(actor_kind="Mlp2", action_limit="Tanh", action_scale=2.0, ent_coef=("Auto", -4.0, 1e-3))


def test_candle_sac_device_noise_equals_the_same_draws_given_by_the_host(B):
    """NULL z: B*A draws for a, then B*A for next_a, from the stream bdr_agent_draw_noise reads."""
    spec = R.CandleSacSpec(12, 4, (64, 64), (64, 64), **SMALL)
    params = spec.init_params(4)
    bsz = 40
    a, b, twin = (_agent(B, spec, bsz, params, seed=17) for _ in range(3))
    for s in range(2):
        batch = R.make_batch(spec, bsz, 60 + s)
        z = twin.draw_noise(2 * bsz * spec.act_dim).reshape(2, bsz, spec.act_dim)
        ra = a.update_on_batch(*batch)
        rb = b.update_on_batch(*batch, z[0], z[1])
        assert ra == rb, s
        for x, y in zip(_state(a, 2), _state(b, 2)):
            assert (bits(x) == bits(y)).all(), s
    # host draws take nothing from b's stream; a's stream moved on by 2 updates x 2 B A
    fresh = _agent(B, spec, bsz, params, seed=17)
    assert (b.draw_noise(16) == fresh.draw_noise(16)).all()
    assert (a.draw_noise(16) == twin.draw_noise(16)).all()
    for x in (a, b, twin, fresh):
        x.close()


def test_candle_sac_two_agents_from_the_same_state_give_the_same_bits(B):
    spec = R.CandleSacSpec(45, 24, (256, 256), (256, 256), n_critics=3, **SMALL)
    params = spec.init_params(9)
    out = []
    for _ in range(2):
        a = _agent(B, spec, 300, params, seed=5)     # device noise: the same seeded stream
        recs = [a.update_on_batch(*R.make_batch(spec, 300, 40 + s)) for s in range(3)]
        out.append((recs, _state(a, 3), a.probe("logp", 300), a.probe("dq_da", 300), a.get_params("actor", "grad")))
        a.close()
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert (bits(x) == bits(y)).all()
    for k in (2, 3, 4):
        assert (bits(out[0][k]) == bits(out[1][k])).all()


def test_candle_sac_eval_mode_update_takes_no_draws_and_the_ent_coef_still_steps(B):
    spec = R.CandleSacSpec(10, 3, (32, 32), (32, 32), actor_kind="Mlp2", action_min=-0.4, action_max=0.5, ent_coef=("Auto", -3.0, 1e-2))
    params = spec.init_params(6)
    a = _agent(B, spec, 24, params, train=False, seed=3)
    ref = R.CandleSacRestatement(spec, *params)
    ref64 = R.CandleSacRestatement(spec, *params, dtype=torch.float64)
    batch = R.make_batch(spec, 24, 7)
    rec = a.update_on_batch(*batch)
    r = ref.update(*batch)     # z = None: the means
    ref64.update(*batch)
    _check_step(a, spec, 24, _want(ref, spec), R.f32_f64_figures(ref, ref64), "eval")
    assert rec["ent_coef"] != 1.0 and a.get_params("log_alpha")[0] != 0.0      # the EntCoef stepped
    _close(rec["ent_coef"], r["ent_coef"], "eval")
    fresh = _agent(B, spec, 24, params, seed=3)
    assert (a.draw_noise(32) == fresh.draw_noise(32)).all()                     # no draws taken
    a.close(); fresh.close()


def test_candle_sac_is_truncated_does_not_change_the_target(B):
    spec = R.CandleSacSpec(9, 3, (32, 32), (32,), actor_kind="Mlp2")
    params = spec.init_params(2)
    obs, act, nxt, rew, _, _ = R.make_batch(spec, 8, 4)
    z = spec.draws(8, 1)
    tg = []
    for trunc in (np.zeros(8, np.int8), np.ones(8, np.int8)):
        a = _agent(B, spec, 8, params)
        a.update_on_batch(obs, act, nxt, rew, np.zeros(8, np.int8), trunc, *z)
        tg.append(a.probe("tgt", 8))
        a.close()
    assert (bits(tg[0]) == bits(tg[1])).all() and not (tg[0] == rew).all()      # gamma_not_done(.., None, ..): sac/base.rs:75-76
    a = _agent(B, spec, 8, params)
    a.update_on_batch(obs, act, nxt, rew, np.ones(8, np.int8), np.zeros(8, np.int8), *z)
    assert (a.probe("tgt", 8) == rew).all()                                      # terminated: gnd = 0, tgt = r exactly
    a.close()


# ---------------------------------------------------------------------------------------------------------- replay, trainers
def _buffer(B, spec, n, seed, capacity=4096):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed), (spec.obs_dim,), np.float32, (spec.act_dim,), np.float32)
    rows = R.make_batch(spec, n, 77)
    rb.push(*rows)
    return rb, rows


def _replay_draws(twin, bsz, A):
    z = twin.draw_noise(2 * bsz * A).reshape(2, bsz, A)
    return z[0], z[1]


def _loose_state(a, ref, spec, tag):
    """free runs on the device's own N(0,1) draws may saturate the Tanh limit: parameters and targets only"""
    assert np.abs(a.get_params("actor") - ref.params("actor")).max() < 0.3 * spec.lr_actor, tag
    for i in range(spec.n_critics):
        assert np.abs(a.get_params(f"critic_{i}") - ref.params(f"critic_{i}")).max() < 0.3 * spec.lr_critic, (tag, i)
        assert rel(a.get_params(f"critic_tgt_{i}"), ref.params(f"critic_tgt_{i}")) < 1e-5, (tag, i)


def test_candle_sac_opt_over_replay_with_three_updates_per_opt(B):
    """Agent::opt over the HBM ring, n_updates_per_opt = 3, train mode on the device stream, against the restatement fed the indices
    of bdr_replay_sample_indices and the draws of a same-seed twin; the 3-key record (the Clamp limit: no saturation to bound)."""
    spec = R.CandleSacSpec(19, 4, (64, 64), (64, 64), actor_kind="Mlp2", ent_coef=("Auto", -4.0, 1e-3))
    params = spec.init_params(3)
    rb, rows = _buffer(B, spec, 1000, 42)
    twin_rb, _ = _buffer(B, spec, 1000, 42)
    a = _agent(B, spec, 64, params, n_updates_per_opt=3, seed=8)
    twin = _agent(B, spec, 64, params, seed=8)
    ref = R.CandleSacRestatement(spec, *params)
    for k in range(2):
        rec = a.opt_with_record(rb)
        assert list(rec) == list(R.RECORD_KEYS)
        rs = []
        for _ in range(3):
            ix = twin_rb.sample_indices(64).astype(np.int64)
            rs.append(ref.update(*[x[ix] for x in rows], *_replay_draws(twin, 64, spec.act_dim)))
        want = ref.opt_record(rs)
        for key in R.RECORD_KEYS:
            _close(rec[key], want[key], (k, key))
        _loose_state(a, ref, spec, k)
    assert a.n_opts == 6
    a.close(); twin.close(); rb.close(); twin_rb.close()


def test_candle_sac_offline_trainer(B):
    """Trainer::train_offline (csrc/trainer.hip) runs N opts of a candle SAC agent; the observer's records are the restatement's."""
    spec = R.CandleSacSpec(12, 3, (32, 32), (32, 32), actor_kind="Mlp2", ent_coef=("Auto", -3.0, 1e-3))
    params = spec.init_params(8)
    rb, rows = _buffer(B, spec, 500, 7)
    twin_rb, _ = _buffer(B, spec, 500, 7)
    a = _agent(B, spec, 32, params, seed=2)
    twin = _agent(B, spec, 32, params, seed=2)
    events = []
    tr = B.NativeTrainer(B.TrainerConfig(max_opts=6, record_agent_info_interval=2))
    st = tr.train_offline(a, rb, on_event=lambda e, o, kind, sc: events.append((o, kind, sc)))
    assert st["opt_steps"] == 6 and a.n_opts == 6
    ref = R.CandleSacRestatement(spec, *params)
    recs = {}
    for o in range(1, 7):
        ix = twin_rb.sample_indices(32).astype(np.int64)
        recs[o] = ref.update(*[x[ix] for x in rows], *_replay_draws(twin, 32, spec.act_dim))
    got = [(o, sc) for o, kind, sc in events if kind == "opt_record"]
    assert [o for o, _ in got] == [2, 4, 6]
    for o, sc in got:
        assert len(sc) == 3
        for key, v in zip(R.RECORD_KEYS, sc):
            _close(float(v), recs[o][key], (o, key))
    _loose_state(a, ref, spec, "offline")
    a.close(); twin.close(); rb.close(); twin_rb.close()


def test_candle_sac_online_trainer_with_a_float_action_env(B):
    """bdr_trainer_train with a candle SAC handle (examples/gym/sac_pendulum's loop): the default function table samples f32 action
    rows and pushes them through the generic act rows."""
    od, ad = 3, 1
    spec = R.CandleSacSpec(od, ad, (64, 64), (64, 64), actor_kind="Mlp2", action_limit="Tanh", action_scale=2.0, ent_coef=("Auto", -1.0, 3e-4))
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=200, seed=9), (od,), np.float32, (ad,), np.float32)
    a = _agent(B, spec, 16, spec.init_params(1), seed=3)
    env = B.SyntheticEnv((od,), np.float32, seed=11, p_term=0.1)
    ev = []
    st = B.NativeTrainer(B.TrainerConfig(max_opts=20, opt_interval=2, warmup_period=24, record_agent_info_interval=5)).train(
        env, a, rb, (od,), np.float32, act_row_bytes=ad * 4, act_dtype=np.float32, on_event=lambda e, o, k, sc: ev.append((e, o, k, sc)))
    a.sync()
    assert st["opt_steps"] == a.n_opts == 20 and st["env_steps"] == rb.len() and 24 + 2 * 19 <= st["env_steps"] <= 24 + 2 * 20
    recs = [sc for _, _, k, sc in ev if k == "opt_record"]
    assert len(recs) == 4 and all(len(sc) == 3 and np.isfinite(sc).all() for sc in recs)
    b = rb.batch(32)
    assert b.act.dtype == np.float32 and (np.abs(b.act) <= 2.0).all() and np.abs(b.act).max() > 0
    assert len(np.unique(b.act)) > 8   # sampled actions, not one constant
    a.close(); rb.close()


# ---------------------------------------------------------------------------------------------------------- acting with Mlp2
@pytest.mark.parametrize("limit", ["Clamp", "Tanh"])
def test_candle_sac_mlp2_acting_layer_path_restatement_and_fused_bits(B, limit):
    """Policy::sample with the Mlp2 actor for n = 1, 33, 300 through sample, sample_device and sample_raw with a normaliser: the layer
    path within 1e-5 of the restatement, BDR_ACT_PATH_FUSED equal to it on the raw bits; eval and train mode (one stream of draws)."""
    O, A = 10, 5
    spec = R.CandleSacSpec(O, A, (48, 96), (8,), actor_kind="Mlp2", action_limit=limit, action_scale=1.5, action_min=-0.3, action_max=0.4)
    params = spec.init_params(6)
    ref = R.CandleSacRestatement(spec, *params)
    k = np.arange(O)
    mean, std = (1000.0 + 0.01 * k).astype(np.float32), (0.5 + 0.25 * (k % 5)).astype(np.float32)
    norm = B.ObsNormalizer(O, 0).set(mean, std)
    for train in (False, True):
        lay, fus, twin = (_agent(B, spec, 4, params, train=train, seed=21) for _ in range(3))
        lay.set_act_path("layers"); fus.set_act_path("fused")
        for n in (1, 33, 300):
            obs = np.random.default_rng(n).standard_normal((n, O)).astype(np.float32)
            dev = torch.full((n, O + 3), float("nan"), dtype=torch.float32, device="cuda")
            dev[:, :O] = torch.from_numpy(obs).cuda()
            torch.cuda.synchronize()
            raw = mean.astype(np.float64) + std.astype(np.float64) * np.random.default_rng(n + 1).standard_normal((n, O))
            zrows = (raw.astype(np.float32) - mean) / std
            calls = (("sample", lambda ag: ag.sample(obs), obs),
                     ("sample_device", lambda ag: ag.sample_device(dev.data_ptr(), n, (O + 3) * 4), obs),
                     ("sample_raw", lambda ag: ag.sample_raw(raw, norm), zrows))
            for name, call, rows in calls:
                al, af = call(lay), call(fus)
                assert al.shape == (n, A) and (bits(al) == bits(af)).all(), (limit, train, n, name)
                z = twin.draw_noise(n * A).reshape(n, A) if train else None
                assert np.abs(al - ref.sample(rows, z)).max() < 1e-5, (limit, train, n, name, np.abs(al - ref.sample(rows, z)).max())
        for x in (lay, fus, twin):
            x.close()
    norm.close()


# ---------------------------------------------------------------------------------------------------------- checkpoints, refusals
def _safetensors_names(path):
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        hdr = json.loads(f.read(n))
    return {k: v["shape"] for k, v in hdr.items() if k != "__metadata__"}


@pytest.mark.parametrize("kind", ["Mlp2", "Mlp3"])
def test_candle_sac_checkpoint_files_names_quirk_and_round_trip(B, tmp_path, kind):
    spec = R.CandleSacSpec(8, 3, (16, 24), (16, 16), actor_kind=kind, ent_coef=("Auto", -3.0, 1e-2))
    a = _agent(B, spec, 32, spec.init_params(1))
    for s in range(2):
        a.update_on_batch(*R.make_batch(spec, 32, s), *spec.draws(32, s))
    files = a.save_params(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["actor.pt", "critic.pt", "critic.tgt.pt", "ent_coef.pt"]
    assert sorted(os.listdir(tmp_path)) == ["actor.pt", "critic.pt", "critic.tgt.pt", "ent_coef.pt"]
    names = _safetensors_names(files[0])
    if kind == "Mlp2":   # mlp2.rs:47-52: the trunk's ln{i}, then the two heads
        assert names == {"actor.mlp.ln0.weight": [16, 8], "actor.mlp.ln0.bias": [16], "actor.mlp.ln1.weight": [24, 16], "actor.mlp.ln1.bias": [24],
                         "actor.mean.weight": [3, 24], "actor.mean.bias": [3], "actor.std.weight": [3, 24], "actor.std.bias": [3]}
    else:
        assert names["actor.head2"] == [1, 3] and names["actor.mlp.ln2.weight"] == [3, 24] and len(names) == 7
    assert set(_safetensors_names(files[1])) == {f"critic{i}.mlp.ln{k}.{t}" for i in range(2) for k in range(3) for t in ("weight", "bias")}
    assert open(files[1], "rb").read() == open(files[2], "rb").read()   # critic.tgt.pt holds the ONLINE critics (util/critic.rs:272-285)
    assert _safetensors_names(files[3]) == {"log_alpha": [1]}
    b = B.CandleSac.build(spec.to_config(B, 32, device=0, seed=99))
    tgt_before = [b.get_params(f"critic_tgt_{i}") for i in range(2)]
    b.load_params(str(tmp_path))
    for m in ("actor", "critic_0", "critic_1", "log_alpha"):
        assert (bits(b.get_params(m)) == bits(a.get_params(m))).all(), m
    assert a.get_params("log_alpha")[0] != 0.0
    for i in range(2):
        assert (b.get_params(f"critic_tgt_{i}") == tgt_before[i]).all()   # load leaves the targets alone
    obs = np.random.default_rng(3).standard_normal((9, 8)).astype(np.float32)
    a.eval(); b.eval()
    assert (bits(a.sample(obs)) == bits(b.sample(obs))).all()            # the same actions after the round trip
    # "<stem>.safetensors" with BDR_CKPT_SAFETENSORS
    d2 = tmp_path / "st"
    a.set_checkpoint_format("safetensors")
    assert [os.path.basename(f) for f in a.save_params(str(d2))] == ["actor.safetensors", "critic.safetensors", "critic.tgt.safetensors", "ent_coef.safetensors"]
    a.close(); b.close()


def test_candle_sac_mlp2_parameter_view_is_the_reference_layout(B):
    """set_params -> get_params is the identity, and the heads land where mlp2.rs puts them: zeroing std.weight and setting std.bias
    makes every row's std exp(clamp(exp(bias)))"""
    spec = R.CandleSacSpec(6, 2, (16, 8), (8,), actor_kind="Mlp2", min_log_std=-5.0, max_log_std=0.5)
    actor, critics, tgts = spec.init_params(2)
    a = _agent(B, spec, 4, (actor, critics, tgts), seed=1)
    assert a.param_count("actor") == spec.actor_count() and (bits(a.get_params("actor")) == bits(actor)).all()
    p = actor.copy()
    A, H = 2, 8
    p[-(A * H + A):-A] = 0.0                  # std.weight
    p[-A:] = np.log([0.25, 3.0])              # std.bias: l = 0.25 (inside), 3.0 (clamped to 0.5)
    a.set_params(p, "actor")
    obs = np.random.default_rng(0).standard_normal((5, 6)).astype(np.float32)
    a.eval(); m = a.sample(obs)
    a.train(); t = a.sample(obs)
    twin = _agent(B, spec, 4, (p, critics, tgts), seed=1)
    z = twin.draw_noise(10).reshape(5, 2)
    sd = np.exp(np.array([0.25, 0.5], np.float32))
    inside = (np.abs(m + sd * z) < 1.0).all(axis=1)
    assert inside.any() and np.abs((t - m)[inside] - (sd * z)[inside]).max() < 1e-5
    a.close(); twin.close()


def test_candle_sac_refusals(B):
    spec = R.CandleSacSpec(8, 3, (16, 16), (16,))
    with pytest.raises(B.BdrError, match="at least 2 rows"):
        B.CandleSac.build(spec.to_config(B, 1, device=0))
    a = _agent(B, spec, 8, spec.init_params(1))
    with pytest.raises(B.BdrError, match="at least 2 rows"):
        a.update_on_batch(*R.make_batch(spec, 1, 2))
    assert a.n_opts == 0
    with pytest.raises(B.BdrError, match="unknown SAC probe|no update"):
        a.probe("tgt", 8)
    a.close()
    cfg = spec.to_config(B, 4, device=0)
    cfg.actor_config.policy_config = B.CandleMlpConfig((16,))        # Mlp2 with one trunk layer
    with pytest.raises(B.BdrError, match="at least 2 layers"):
        B.CandleSac.build(cfg)
    for act in ("Tanh", "Sigmoid"):   # activation_out Tanh / Sigmoid: not supported
        cfg = spec.to_config(B, 4, device=0)
        cfg.critic_config.q_config = B.CandleMlpConfig((16,), act)
        with pytest.raises(B.BdrError):
            B.CandleSac.build(cfg)
    for which in ("critic_config", "actor_config"):
        cfg = spec.to_config(B, 4, device=0)
        getattr(cfg, which).opt_config = B.OptimizerConfig.AdamW(1e-3, amsgrad=True)   # candle's AdamW has no amsgrad
        with pytest.raises(B.BdrError, match="amsgrad"):
            B.CandleSac.build(cfg)
    cfg = spec.to_config(B, 4, device=0)
    cfg.ent_coef_mode = B.EntCoefMode.Fix(0.0)
    with pytest.raises(B.BdrError, match="alpha > 0"):
        B.CandleSac.build(cfg)
    # the tch SAC's entry points refuse this handle and the other way round
    L = B._lib.lib()
    a = B.CandleSac.build(spec.to_config(B, 4, device=0))
    out = np.zeros(3, np.float32)
    assert L.bdr_sac_sample(a.handle, 1, np.zeros(8, np.float32).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 1
    # synchronous data-parallel gradients: refused for a candle SAC handle
    uid = (C.c_uint8 * B._lib.BDR_UNIQUE_ID_BYTES)()
    B._lib.check(L.bdr_comm_get_unique_id(uid))
    h = C.c_void_p()
    B._lib.check(L.bdr_comm_init_rank(uid, 1, 0, 0, C.byref(h)))
    assert L.bdr_agent_set_grad_comm(a.handle, h) == 1   # BDR_ERR_INVALID
    assert b"candle SAC" in L.bdr_last_error()
    a.close()
    B._lib.check(L.bdr_comm_destroy(h))
