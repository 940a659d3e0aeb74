"""HIP BC agent (csrc/bc.hip, through the C ABI) against the committed goldens and the float32 autograd restatement of
border-candle-agent's Bc::opt_ (tests/bc_restatement.py), in both kernel forms where the form applies.  Tolerances are those of
tests/test_gpu_iql.py / test_gpu_awac.py: parameters within 0.3 lr of the restatement after each step, gradients within 2e-3 relative,
the loss within 5e-4 |want| + 1e-6, probes within 1e-4 relative."""
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
import bc_restatement as R  # noqa: E402
import make_golden_bc as MG  # noqa: E402

FORMS = ("general", "fused", "fused_mfma")
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)


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
    a = B.Bc.build(spec.to_config(B, bsz, device=0, **kw))
    a.set_params(params)
    return a


def _close(x, want, tag):
    print(tag, "loss", x, "want", want)
    assert abs(x - want) <= 5e-4 * abs(want) + 1e-6, (tag, x, want)


def _check_step(a, spec, bsz, rec, want_loss, want_pred, want_dz, want_grad, want_params, tag):
    _close(rec["loss"], want_loss, tag)
    figs = (rel(a.probe("pred", bsz), want_pred), rel(a.probe("dz", bsz), want_dz), rel(a.get_params(role="grad"), want_grad),
            np.abs(a.get_params() - want_params).max() / spec.lr)
    print(tag, "pred rel %.3g  dz rel %.3g  grad rel %.3g  param step / lr %.3g" % figs)
    assert figs[0] < 1e-4 and figs[1] < 1e-4, (tag, figs)
    assert figs[2] < 2e-3, (tag, figs)
    assert figs[3] < 0.3, (tag, figs)


# ---------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_bc_goldens(B, golden_dir, name, form):
    spec, bsz, steps, seed = MG.case(name)
    g = np.load(os.path.join(golden_dir, f"bc_{name}.npz"))
    a = _agent(B, spec, bsz, g["policy0"], kernel_form=form)
    for s in range(steps):
        rec = a.update_on_batch(g[f"s{s}_obs"], g[f"s{s}_act"])
        _check_step(a, spec, bsz, rec, float(g[f"s{s}_loss"]), g[f"s{s}_pred"], g[f"s{s}_dz"], g[f"s{s}_grad"], g[f"s{s}_policy"], (name, form, s))
    assert a.n_opts == steps
    a.close()


# ---------------------------------------------------------------------------------------------------------- restatement
def _free_run(B, spec, bsz, steps, seed, **kw):
    params = spec.init_params(seed)
    a = _agent(B, spec, bsz, params, **kw)
    ref = R.BcRestatement(spec, params)
    for s in range(steps):
        batch = R.make_batch(spec, bsz, seed * 100 + s)
        rec = a.update_on_batch(*batch)
        r = ref.update(*batch)
        _check_step(a, spec, bsz, rec, r["loss"], ref.probes["pred"], ref.probes["dz"], ref.probes["grad"], ref.params(), (kw, s))
    assert a.n_opts == steps
    return a, ref


@pytest.mark.parametrize("form,rows", [("general", 0), ("fused", 0), ("fused", 16), ("fused", 32), ("fused_mfma", 0), ("default", 0)])
def test_bc_pen_shape_against_the_restatement(B, form, rows):
    """examples/d4rl/bc_pen: obs 45, act 24, [256, 256] with a Tanh output, B = 256; five free-running updates."""
    spec = R.BcSpec(45, 24, (256, 256), "Tanh", lr=1e-3, adamw=ADAMW)
    a, _ = _free_run(B, spec, 256, 5, 11, kernel_form=form, head_rows=rows)
    a.close()


RAGGED = [
    # obs, act, units, activation_out, batch, forms
    (17, 6, (64, 48), "None", 7, FORMS),
    (70, 5, (100,), "Sigmoid", 300, FORMS),
    (33, 13, (96, 80, 72), "ReLU", 129, FORMS),
    (3, 1, (64, 64), "Tanh", 1, FORMS),
    (45, 64, (320,), "Tanh", 33, FORMS),             # a full column block, a hidden width that is not a multiple of 256
    (21, 65, (64, 40), "Tanh", 50, ("general",)),     # out_dim 65 and above: the general form only
    (12, 130, (72,), "Sigmoid", 260, ("general",)),
    (9, 4, (), "None", 20, ("general",)),             # no hidden layer
]


@pytest.mark.parametrize("od,ad,units,act_out,bsz,forms", RAGGED)
def test_bc_ragged_shapes(B, od, ad, units, act_out, bsz, forms):
    for form in forms:
        spec = R.BcSpec(od, ad, units, act_out, lr=1e-3, adamw=ADAMW if bsz % 2 else None)
        a, _ = _free_run(B, spec, bsz, 3, 5, kernel_form=form)
        a.close()


def test_bc_a_forced_fused_head_is_refused_where_it_does_not_apply(B):
    for od, ad, units in ((21, 65, (64,)), (9, 4, ()), (9, 4, (1024,))):
        spec = R.BcSpec(od, ad, units, "Tanh")
        for form in ("fused",) + (("fused_mfma",) if ad > 64 or not units else ()):
            with pytest.raises(B.BdrError, match="BDR_BC_KERNEL_GENERAL"):
                B.Bc.build(spec.to_config(B, 8, device=0, kernel_form=form))
        B.Bc.build(spec.to_config(B, 8, device=0, kernel_form="default")).close()   # the default falls to the general form


@pytest.mark.parametrize("form", FORMS)
def test_bc_replay_and_two_agents_give_the_same_bits(B, form):
    spec = R.BcSpec(45, 24, (256, 256), "Tanh", lr=1e-3, adamw=ADAMW)
    params = spec.init_params(9)
    out = []
    for _ in range(3):     # two agents side by side would be the same launches: a third run is the replay
        a = _agent(B, spec, 300, params, kernel_form=form)
        recs = [a.update_on_batch(*R.make_batch(spec, 300, 40 + s)) for s in range(3)]
        out.append((recs, a.get_params(), a.get_params(role="exp_avg_sq"), a.probe("pred", 300), a.probe("dz", 300)))
        a.close()
    for k in (1, 2):
        assert out[0][0] == out[k][0]
        for x, y in zip(out[0][1:], out[k][1:]):
            assert (x == y).all()


# ---------------------------------------------------------------------------------------------------------- replay, trainers
def _rows(spec, n, seed):
    obs, act = R.make_batch(spec, n, seed)
    rng = np.random.default_rng(seed + 1)
    return obs, act, rng.standard_normal((n, spec.obs_dim)).astype(np.float32), rng.standard_normal(n).astype(np.float32), \
        np.zeros(n, np.int8), np.zeros(n, np.int8)


def _buffer(B, spec, n, seed, capacity=4096):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed), (spec.obs_dim,), np.float32, (spec.act_dim,), np.float32)
    rows = _rows(spec, n, 77)
    rb.push(*rows)
    return rb, rows


@pytest.mark.parametrize("form", FORMS)
def test_bc_opt_over_replay_equals_update_on_batch_on_the_ring_rows(B, form):
    """Agent::opt over the HBM ring == update_on_batch on the rows bdr_replay_sample_indices selects (a same-seed twin ring), bit for
    bit, and the one-key record."""
    spec = R.BcSpec(19, 4, (64, 64), "Tanh")
    params = spec.init_params(3)
    rb, rows = _buffer(B, spec, 1000, 42)
    twin_rb, _ = _buffer(B, spec, 1000, 42)
    a = _agent(B, spec, 64, params, kernel_form=form)
    b = _agent(B, spec, 64, params, kernel_form=form)
    ref = R.BcRestatement(spec, params)
    for k in range(3):
        rec = a.opt_with_record(rb)
        assert list(rec) == ["loss"]
        ix = twin_rb.sample_indices(64).astype(np.int64)
        rb_ = b.update_on_batch(rows[0][ix], rows[1][ix])
        r = ref.update(rows[0][ix], rows[1][ix])
        assert rec["loss"] == rb_["loss"], k
        assert (a.get_params() == b.get_params()).all(), k
        _close(rec["loss"], r["loss"], ("ring", k))
        assert np.abs(a.get_params() - ref.params()).max() < 0.3 * spec.lr
    assert a.n_opts == 3
    a.close(); b.close(); rb.close(); twin_rb.close()


def test_bc_offline_trainer(B):
    """Trainer::train_offline (csrc/trainer.hip) runs N opts of a BC agent == N manual updates on the ring's index stream."""
    spec = R.BcSpec(12, 3, (32, 32), "Tanh")
    params = spec.init_params(8)
    rb, rows = _buffer(B, spec, 500, 7)
    twin_rb, _ = _buffer(B, spec, 500, 7)
    a = _agent(B, spec, 32, params)
    b = _agent(B, spec, 32, params)
    events = []
    tr = B.NativeTrainer(B.TrainerConfig(max_opts=6, record_agent_info_interval=2))
    st = tr.train_offline(a, rb, on_event=lambda e, o, kind, sc: events.append((o, kind, sc)))
    assert st["opt_steps"] == 6 and a.n_opts == 6
    recs = {}
    for o in range(1, 7):
        ix = twin_rb.sample_indices(32).astype(np.int64)
        recs[o] = b.update_on_batch(rows[0][ix], rows[1][ix])
    got = [(o, sc) for o, kind, sc in events if kind == "opt_record"]
    assert [o for o, _ in got] == [2, 4, 6]
    for o, sc in got:
        assert len(sc) == 1 and sc[0] == np.float32(recs[o]["loss"])
    assert (a.get_params() == b.get_params()).all()
    a.close(); b.close(); rb.close(); twin_rb.close()


def test_bc_online_trainer_with_a_float_action_env(B):
    """bdr_trainer_train with a BC handle: the default function table samples f32 action rows through the agent's sample_f32."""
    od, ad = 3, 2
    spec = R.BcSpec(od, ad, (64, 64), "Tanh")
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=200, seed=9), (od,), np.float32, (ad,), np.float32)
    a = _agent(B, spec, 16, spec.init_params(1))
    env = B.SyntheticEnv((od,), np.float32, seed=11, p_term=0.1)
    ev = []
    st = B.NativeTrainer(B.TrainerConfig(max_opts=20, opt_interval=2, warmup_period=24, record_agent_info_interval=5)).train(
        env, a, rb, (od,), np.float32, act_row_bytes=ad * 4, act_dtype=np.float32, on_event=lambda e, o, k, sc: ev.append((e, o, k, sc)))
    a.sync()
    assert st["opt_steps"] == a.n_opts == 20 and st["env_steps"] == rb.len()
    recs = [sc for _, _, k, sc in ev if k == "opt_record"]
    assert len(recs) == 4 and all(len(sc) == 1 and np.isfinite(sc).all() for sc in recs)
    b = rb.batch(32)
    assert b.act.dtype == np.float32 and (np.abs(b.act) <= 1.0).all() and np.abs(b.act).max() > 0
    assert len(np.unique(b.act)) > 8   # the policy's outputs, not one constant
    assert not a.is_train()            # the trainer called train(): accepted, and is_train() stays false (bc/base.rs:104-112)
    a.close(); rb.close()


def test_bc_async_actors_sample_bc_actions(B):
    od, ad, n_act, max_opts, warm = 5, 2, 2, 20, 96
    spec = R.BcSpec(od, ad, (64, 64), "Tanh")
    learner = _agent(B, spec, 32, spec.init_params(1))
    actors = [_agent(B, spec, 32, spec.init_params(10 + i)) for i in range(n_act)]
    envs = [B.SyntheticEnv((od,), np.float32, seed=i, p_term=0.1) for i in range(n_act)]
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=500, seed=42), (od,), np.float32, (ad,), np.float32)
    events = []
    tr = B.AsyncTrainer(B.AsyncTrainerConfig(max_opts=max_opts, warmup_period=warm, sync_interval=5, record_agent_info_interval=10,
                                             record_compute_cost_interval=0, warmup_sleep_ms=5), B.ActorManagerConfig(n_buffer=16))
    st = tr.train(learner, rb, actors, envs, (od,), np.float32, act_row_bytes=ad * 4, act_dtype=np.float32, on_event=lambda *e: events.append(e))
    assert st.opt_steps == max_opts and learner.n_opts == max_opts
    recs = [e for e in events if e[3] == "opt_record"]
    assert len(recs) == max_opts // 10 and all(len(e[4]) == 1 and np.isfinite(e[4]).all() for e in recs)
    b = rb.batch(64)
    assert b.act.dtype == np.float32 and b.act.shape == (64, ad) and (np.abs(b.act) <= 1.0).all() and np.abs(b.act).max() > 0
    synced = {e[0]: e[2] for e in events if e[3] == "actor_sync"}
    for i, x in enumerate(actors):
        if synced.get(i) == max_opts:
            assert (x.get_params() == learner.get_params()).all()
    assert any(v > 0 for v in synced.values())
    for x in actors:
        x.close()
    learner.close(); rb.close()


# ---------------------------------------------------------------------------------------------------------- sample, checkpoints, rejects
@pytest.mark.parametrize("act_out", ["None", "ReLU", "Tanh", "Sigmoid"])
def test_bc_sample_continuous_is_the_forward_output(B, act_out):
    spec = R.BcSpec(10, 4, (32, 32), act_out)
    params = spec.init_params(6)
    a = _agent(B, spec, 16, params)
    ref = R.BcRestatement(spec, params)
    obs = np.random.default_rng(1).standard_normal((9, 10)).astype(np.float32)
    e1, e2 = a.sample(obs), a.sample(obs)
    assert e1.dtype == np.float32 and e1.shape == (9, 4) and (e1 == e2).all()
    assert np.abs(e1 - ref.sample(obs)).max() < 1e-5
    a.train()
    assert not a.is_train() and (a.sample(obs) == e1).all()    # no train mode, no noise
    # the update's probe of the same rows is the same forward
    rec = a.update_on_batch(obs, np.zeros((9, 4), np.float32))
    assert np.abs(a.probe("pred", 9) - e1).max() < 1e-5 and np.isfinite(rec["loss"])
    a.close()


@pytest.mark.parametrize("act_out", ["None", "Tanh"])
def test_bc_sample_discrete_is_the_argmax(B, act_out):
    spec = R.BcSpec(10, 6, (32, 32), act_out, action_type="Discrete")
    params = spec.init_params(6)
    ref = R.BcRestatement(spec, params)
    obs = np.random.default_rng(5).standard_normal((200, 10)).astype(np.float32)   # (a seed chosen on the CPU for the precondition below)
    y = ref.forward(obs).detach().numpy()
    top2 = np.sort(y, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] > 1e-4).all()    # the precondition: no row has its two largest outputs within 1e-4
    a = _agent(B, spec, 16, params)
    idx = a.sample(obs)
    assert idx.dtype == np.int64 and idx.shape == (200,)
    assert (idx == y.argmax(1)).all() and (idx == ref.sample(obs)).all()
    a.close()


def test_bc_discrete_ties_take_the_lowest_index(B):
    """a ReLU output that is 0 everywhere ties in every row: index 0 (the kernel's documented order)"""
    spec = R.BcSpec(5, 4, (8,), "ReLU", action_type="Discrete")
    p = spec.init_params(1)
    p[-4:] = -100.0          # the last layer's bias: every pre-activation far below 0
    a = _agent(B, spec, 4, p)
    assert (a.sample(np.random.default_rng(0).standard_normal((7, 5)).astype(np.float32)) == 0).all()
    a.close()


def test_bc_host_rows_equal_device_rows(B):
    from border_amd import _lib
    spec = R.BcSpec(4, 3, (64, 64), "Tanh")
    rb, _ = _buffer(B, spec, 40, 1, capacity=64)
    b = rb.batch(16)
    db = _lib.DeviceBatch()
    _lib.check(_lib.lib().bdr_replay_last_batch(rb.handle, C.byref(db)))
    a = _agent(B, spec, 8, spec.init_params(2))
    assert (a.sample(b.obs) == a.sample_device(db.obs, 16, 16)).all()
    d = B.Bc.build(R.BcSpec(4, 3, (64, 64), "Tanh", action_type="Discrete").to_config(B, 8, device=0))
    d.set_params(spec.init_params(2))
    assert (d.sample(b.obs) == d.sample_device(db.obs, 16, 16)).all()
    a.close(); d.close(); rb.close()


def _safetensors_names(path):
    with open(path, "rb") as f:
        n = struct.unpack("<Q", f.read(8))[0]
        hdr = json.loads(f.read(n))
    return {k: v["shape"] for k, v in hdr.items() if k != "__metadata__"}


def test_bc_checkpoint_file_names_and_round_trip(B, tmp_path):
    spec = R.BcSpec(8, 3, (16, 12), "Tanh")
    a = _agent(B, spec, 32, spec.init_params(1))
    for s in range(2):
        a.update_on_batch(*R.make_batch(spec, 32, s))
    files = a.save_params(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["policy_model.pt"] and sorted(os.listdir(tmp_path)) == ["policy_model.pt"]
    names = _safetensors_names(files[0])
    assert names == {"mlp.ln0.weight": [16, 8], "mlp.ln0.bias": [16], "mlp.ln1.weight": [12, 16], "mlp.ln1.bias": [12],
                     "mlp.ln2.weight": [3, 12], "mlp.ln2.bias": [3]}
    b = B.Bc.build(spec.to_config(B, 32, device=0, seed=99))
    assert not (b.get_params() == a.get_params()).all()
    b.load_params(str(tmp_path))
    assert (b.get_params() == a.get_params()).all()
    a.set_checkpoint_format("safetensors")
    other = tmp_path / "st"
    assert [os.path.basename(f) for f in a.save_params(str(other))] == ["policy_model.safetensors"]
    c = B.Bc.build(spec.to_config(B, 32, device=0, seed=98))
    c.load_params(str(other))      # the load path falls back to the other extension
    assert (c.get_params() == a.get_params()).all()
    a.close(); b.close(); c.close()


def test_bc_loads_a_file_written_by_the_safetensors_package(B, tmp_path):
    from safetensors.numpy import save_file
    spec = R.BcSpec(8, 3, (16,), "Sigmoid")
    flat = spec.init_params(4)
    tensors, o = {}, 0
    for k, (i_, o_) in enumerate(((8, 16), (16, 3))):
        tensors[f"mlp.ln{k}.weight"] = flat[o:o + i_ * o_].reshape(o_, i_).copy(); o += i_ * o_
        tensors[f"mlp.ln{k}.bias"] = flat[o:o + o_].copy(); o += o_
    save_file(tensors, str(tmp_path / "policy_model.pt"))
    a = B.Bc.build(spec.to_config(B, 8, device=0, seed=3))
    a.load_params(str(tmp_path))
    assert (a.get_params() == flat).all()
    a.close()


def test_bc_rejects(B):
    spec = R.BcSpec(8, 3, (16,), "Tanh", action_type="Discrete")
    d = _agent(B, spec, 4, spec.init_params(1))          # create works for Discrete
    with pytest.raises(B.BdrError, match="bc/base.rs:174"):
        d.update_on_batch(*R.make_batch(spec, 4, 1))
    rb, _ = _buffer(B, spec, 40, 1, capacity=64)
    with pytest.raises(B.BdrError, match="bc/base.rs:174"):
        d.opt(rb)
    assert d.n_opts == 0
    d.close(); rb.close()
    cfg = R.BcSpec(8, 3, (16,), "Tanh").to_config(B, 4, device=0)
    cfg.policy_model_config.opt_config = B.OptimizerConfig.AdamW(1e-3, amsgrad=True)   # candle's AdamW has no amsgrad
    with pytest.raises(B.BdrError):
        B.Bc.build(cfg)
    # synchronous data-parallel gradients: refused for a BC handle
    L = B._lib.lib()
    uid = (C.c_uint8 * B._lib.BDR_UNIQUE_ID_BYTES)()
    B._lib.check(L.bdr_comm_get_unique_id(uid))
    h = C.c_void_p()
    B._lib.check(L.bdr_comm_init_rank(uid, 1, 0, 0, C.byref(h)))
    a = B.Bc.build(R.BcSpec(8, 3, (16,), "Tanh").to_config(B, 4, device=0))
    assert L.bdr_agent_set_grad_comm(a.handle, h) == 1   # BDR_ERR_INVALID
    assert b"BC" in L.bdr_last_error()
    a.close()
    B._lib.check(L.bdr_comm_destroy(h))
