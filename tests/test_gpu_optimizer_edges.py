"""The optimizer step and the soft update of every agent, element by element, against tests/optimizer_inputs.py.

Per case: build the agent, run t - 1 warm-up updates (the bias corrections are then those of step t), write crafted parameters, moments
and targets, read them back (set -> get round-trips the bits), run ONE update, read the device's own gradient and the state after.  Every
element of every tensor of every model must then carry the bits of adam_f32 / track_f32 applied to the read-back gradient, and lie within
the float64 bar (adam_bars / track_bar) of adam_f64 / track_f64.  Nothing is compared through a maximum over a network.
The cases, the kernels they reach and what the first hardware run found: DESIGN.md section 16.
"""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimizer_inputs as X  # noqa: E402

ENV_KEYS = ("BDR_NO_SAC_FUSE", "BDR_NO_MLP_LDS", "BDR_NO_MLP_FUSED", "BDR_NO_SMALL_GEMM", "BDR_STEP_GRAPH", "BDR_NO_STEP_GRAPH", "BDR_SAC_SIDE_QUEUE",
            "BDR_NO_STEP_GATHER", "BDR_NO_MLP_HEAD_FUSE", "BDR_NO_SAC_CHAIN")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oc(B, o: X.Opt):
    return B.OptimizerConfig.AdamW(o.lr, o.b1, o.b2, o.wd, o.eps, o.amsgrad) if o.adamw else B.OptimizerConfig.Adam(o.lr)


def _dims(c):
    sh = X.SHAPES[c.shape]
    return sh["obs"], sh["act"], tuple(sh["units"])


TARGET_ENTROPY = -3.0
ENT_LR = 3e-4


def build(B, c: X.Case, **kw):
    od, ad, u = _dims(c)
    o = c.opts
    mlp = lambda: B.CandleMlpConfig(u)
    if c.agent == "sac":
        ent = ("Auto", TARGET_ENTROPY, ENT_LR) if c.x("ent") == "auto" else ("Fix", 0.2)
        return B.Sac.build(B.SacConfig(obs_dim=od, act_dim=ad, pi_units=u, q_units=u, opt_actor=_oc(B, o["actor"]), opt_critic=_oc(B, o["critic"]),
                                       tau=c.tau, ent_coef_mode=ent, n_critics=c.nc, batch_size=X.BATCH, device=0, seed=3, **kw))
    if c.agent in ("candle_sac", "iql", "awac"):
        actor = B.GaussianActorConfig(mlp(), _oc(B, o["actor"]), action_limit=B.ActionLimit.Tanh(1.0) if c.agent == "candle_sac" else B.ActionLimit.Clamp(-1.0, 1.0),
                                      kind=c.x("actor", "Mlp3"))
        critic = B.MultiCriticConfig(c.nc, mlp(), _oc(B, o["critic"]), c.tau)
        if c.agent == "candle_sac":
            ent = B.EntCoefMode.Auto(TARGET_ENTROPY, ENT_LR) if c.x("ent") == "auto" else B.EntCoefMode.Fix(0.2)
            return B.CandleSac.build(B.CandleSacConfig(obs_dim=od, act_dim=ad, actor_config=actor, critic_config=critic, ent_coef_mode=ent,
                                                       batch_size=X.BATCH, train=True, device=0, seed=3, **kw))
        if c.agent == "iql":
            return B.Iql.build(B.IqlConfig(obs_dim=od, act_dim=ad, value_config=B.ValueConfig(mlp(), _oc(B, o["value"])), critic_config=critic,
                                           actor_config=actor, batch_size=X.BATCH, train=True, device=0, seed=3, **kw))
        return B.Awac.build(B.AwacConfig(obs_dim=od, act_dim=ad, actor_config=actor, critic_config=critic, batch_size=X.BATCH, train=True, device=0, seed=3, **kw))
    if c.agent == "bc":
        return B.Bc.build(B.BcConfig(obs_dim=od, act_dim=ad, policy_model_config=B.BcModelConfig(mlp(), _oc(B, o["policy"])), batch_size=X.BATCH,
                                     action_type=B.BcActionType.Continuous, device=0, kernel_form=c.x("form", "default")))
    if c.agent in ("dqn_mlp", "dqn_cnn"):
        q = B.MlpConfig(in_dim=od, units=u, out_dim=X.N_ACTIONS) if c.agent == "dqn_mlp" else B.AtariCnnConfig(n_stack=4, out_dim=c.x("actions"))
        kw.setdefault("soft_update_interval", 1)
        return B.Dqn.build(B.DqnConfig(model_config=B.DqnModelConfig(q_config=q, opt_config=_oc(B, o["q"])), batch_size=CNN_BATCH if c.agent == "dqn_cnn" else X.BATCH,
                                       critic_loss="SmoothL1", tau=c.tau, device=0, **kw))
    if c.agent == "iqn":
        f = B.MlpConfig(in_dim=od, units=u, out_dim=X.IQN_FEATURES, activation_out=True)
        kw.setdefault("soft_update_interval", 1)
        return B.Iqn.build(B.IqnConfig(f_config=f, feature_dim=X.IQN_FEATURES, embed_dim=X.IQN_EMBED, m_units=X.IQN_MERGE, n_actions=X.N_ACTIONS,
                                       opt_config=_oc(B, o["q"]), batch_size=X.BATCH, tau=c.tau, device=0, **kw))
    raise KeyError(c.agent)


CNN_BATCH = 4


def models(c: X.Case):
    """[(model, optimizer group, its target or None)] of every network the update steps"""
    if c.agent == "sac":
        return [("pi", "actor", None)] + [(f"qnet_{i}", "critic", f"qnet_tgt_{i}") for i in range(c.nc)]
    if c.agent in ("candle_sac", "iql", "awac"):
        out = [("actor", "actor", None)] + [(f"critic_{i}", "critic", f"critic_tgt_{i}") for i in range(c.nc)]
        return out + ([("value", "value", None)] if c.agent == "iql" else [])
    if c.agent == "bc":
        return [("policy", "policy", None)]
    if c.agent == "iqn":
        return [("iqn", "q", "iqn_tgt")]
    return [("qnet", "q", "qnet_tgt")]


def get(a, c, model, role="param"):
    if c.agent in ("dqn_mlp", "dqn_cnn", "iqn"):
        return a.get_params(model if role == "param" else role)
    return a.get_params(model, role)


def put(a, c, x, model, role="param"):
    if c.agent in ("dqn_mlp", "dqn_cnn", "iqn"):
        return a.set_params(np.asarray(x, np.float32), model if role == "param" else role)
    return a.set_params(x, model, role)


def make(c, rng):
    od, ad, _ = _dims(c)
    if c.agent == "dqn_cnn":
        from oracle import torch_ref as T
        return dict(cnn=T.synthetic_atari_batch(CNN_BATCH, c.x("actions"), int(rng.integers(1 << 30))))
    b = X.make_batch(rng, X.BATCH, od, ad, X.N_ACTIONS if c.agent in ("dqn_mlp", "iqn") else 0)
    if c.agent == "iqn":
        b["tp"], b["tt"] = rng.random((X.BATCH, 8), dtype=np.float32), rng.random((X.BATCH, 8), dtype=np.float32)
    return b


def step(a, c, b):
    if c.agent == "sac":
        return a.update_on_batch(b["obs"], b["act"], b["next_obs"], b["reward"], b["term"], b["z1"], b["z2"])
    if c.agent in ("candle_sac", "awac"):
        return a.update_on_batch(b["obs"], b["act"], b["next_obs"], b["reward"], b["term"], b["trunc"], b["z1"], b["z2"])
    if c.agent == "iql":
        return a.update_on_batch(b["obs"], b["act"], b["next_obs"], b["reward"], b["term"], b["trunc"])
    if c.agent == "bc":
        return a.update_on_batch(b["obs"], b["act"])
    if c.agent == "dqn_cnn":
        return a.update_on_batch(*b["cnn"])
    if c.agent == "dqn_mlp":
        return a.update_on_batch(b["obs"], b["act"], b["next_obs"], b["reward"], b["term"])
    return a.update_on_batch(b["obs"], b["act"], b["next_obs"], b["reward"], b["term"], b["tp"], b["tt"])


def forward_is_finite(a, c, b):
    if c.agent in ("sac", "candle_sac", "iql", "awac", "bc"):
        return np.isfinite(np.asarray(a.sample(b["obs"]), np.float64)).all()
    if c.agent == "dqn_cnn":
        return np.isfinite(a.qvalues(b["cnn"][0])).all()
    if c.agent == "dqn_mlp":
        return np.isfinite(a.qvalues(b["obs"])).all()
    return np.isfinite(a.forward(b["obs"], b["tp"], "iqn")).all()


def same_bits(tag, got, want):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (tag, "elements differ:", bad.size, "of", np.size(got), "first", int(bad[0]), float(np.ravel(got)[bad[0]]), float(np.ravel(want)[bad[0]]))


def within(tag, got, ref64, bar):
    d = np.abs(np.asarray(got, np.float64) - ref64)
    bad = np.flatnonzero(~(d <= bar))
    assert bad.size == 0, (tag, "elements past the bar:", bad.size, "first", int(bad[0]), float(d[bad[0]]), float(bar[bad[0]]))


def check_adam(tag, before, g, after, s):
    """before / after: dict(p, m, v, vmax or None) of one model; g: the device's own gradient of the step between them.
    exp_avg, exp_avg_sq, max_exp_avg_sq: the restatement's bits.  p': the bits of the restatement with the root at one of X.SQRT_ULPS
    (the hardware's square root is accurate to one ulp, X.adam_f32), element by element."""
    args = (before["p"], g, before["m"], before["v"], before["vmax"], s)
    want = X.adam_f32(*args)
    (r64, _), bars = X.adam_f64(*args), X.adam_bars(*args)
    for k, w, r in zip(("p", "m", "v", "vmax"), want, r64):
        if w is None:
            continue
        assert np.isfinite(after[k]).all(), (tag, k)
        if k == "p":
            forms = [bits(X.adam_f32(*args, sqrt_ulps=u)[0]) for u in X.SQRT_ULPS]
            hit = [bits(after[k]) == f for f in forms]
            bad = np.flatnonzero(~(hit[0] | hit[1] | hit[2]))
            print(tag, "p': elements off the rounded root's bits", int((~hit[0]).sum()), "of", w.size)
            assert bad.size == 0, (tag, k, "elements differ:", bad.size, "of", w.size, "first", int(bad[0]), float(after[k][bad[0]]), float(w[bad[0]]))
        else:
            same_bits((tag, k), after[k], w)
        within((tag, k), after[k], r, bars[k])


def check_track(tag, src_after, tgt_before, tgt_after, tau):
    t32, o32 = X.tau_scalars(tau)
    same_bits((tag, "target"), tgt_after, X.track_f32(src_after, tgt_before, t32, o32))
    within((tag, "target"), tgt_after, X.track_f64(src_after, tgt_before, t32, o32), X.track_bar(src_after, tgt_before, t32, o32))
    if tau == 1.0:
        nz = np.asarray(src_after) != 0          # (1 * -0 + 0 * x is +0: a zero's sign is the one thing tau = 1 does not copy)
        same_bits((tag, "tau 1: the source's bits"), np.asarray(tgt_after)[nz], np.asarray(src_after)[nz])
    if tau == 0.0:
        same_bits((tag, "tau 0: its own bits"), tgt_after, tgt_before)


def snapshot(a, c, amsgrad_of):
    out = {}
    for name, group, tgt in models(c):
        out[name] = dict(p=get(a, c, name), m=get(a, c, name, "exp_avg"), v=get(a, c, name, "exp_avg_sq"),
                         vmax=get(a, c, name, "max_exp_avg_sq") if amsgrad_of[group] else None)
        if tgt:
            out[tgt] = get(a, c, tgt)
    return out


def log_alpha_state(a):
    return {k: a.get_params("log_alpha", r) for k, r in (("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq"))}


def check_log_alpha(a, c, before, t):
    """The entropy coefficient's own optimizer, at its own counter.  candle SAC exposes the gradient; the tch SAC does not: its gradient
    is -(mean(log_p) + target_entropy) of the probed log-probabilities, known up to the order of the kernel's sum, so SOME f32 within
    64 ulp of the float64 mean must reproduce exp_avg, exp_avg_sq and log_alpha together, bit for bit, in ONE of the forms the step's
    inline code may have been compiled to (X.log_alpha_step_f32)."""
    o = X.case_configs(c)["log_alpha"]
    s = X.scalars_of(o, t, ENT_LR)
    after = log_alpha_state(a)
    b = dict(before, vmax=None)
    if c.agent == "candle_sac":
        g = a.get_params("log_alpha", "grad")
        check_adam((c.name, "log_alpha"), b, g, dict(after, vmax=None), s)
        return
    est = np.float32(-(np.asarray(a.probe("log_p", X.BATCH), np.float64).mean() + TARGET_ENTROPY))
    cand = [est]
    for d in (np.float32(np.inf), np.float32(-np.inf)):
        x = est
        for _ in range(64):
            x = np.nextafter(x, d)
            cand.append(x)
    cand = np.asarray(cand, np.float32)
    n = cand.size
    hit, forms = np.zeros(n, bool), []
    for form in X.LOG_ALPHA_FORMS:
        rp, rm, rv = X.log_alpha_step_f32(np.repeat(b["p"], n), cand, np.repeat(b["m"], n), np.repeat(b["v"], n), s, form)
        h = (bits(rp) == bits(after["p"])[0]) & (bits(rm) == bits(after["m"])[0]) & (bits(rv) == bits(after["v"])[0])
        if h.any():
            forms.append(form)
        hit |= h
    print(c.name, "log_alpha: gradient estimate", float(est), "matching candidates", int(hit.sum()), "of", n, "forms", forms,
          "after", [float(after[k][0]) for k in "pmv"])
    assert hit.any(), (c.name, "no gradient within 64 ulp of", float(est), "and no form of the step reproduce log_alpha, exp_avg and exp_avg_sq together")
    (r64, _), bars = X.adam_f64(b["p"], cand[hit][:1], b["m"], b["v"], None, s), X.adam_bars(b["p"], cand[hit][:1], b["m"], b["v"], None, s)
    for k, r in zip("pmv", r64):
        within((c.name, "log_alpha", k), after[k], r, bars[k])


def run_case(B, c: X.Case, mp):
    for k in ENV_KEYS:
        mp.delenv(k, raising=False)
    for k, v in c.env:
        mp.setenv(k, v)
    if c.refusal:
        with pytest.raises(B.BdrError) as e:
            build(B, c).close()
        assert c.refusal in str(e.value), str(e.value)
        return
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    nets, sh = X.model_nets(c), X.SHAPES[c.shape]
    ams = {g: o.amsgrad for g, o in c.opts.items()}
    auto = c.x("ent") == "auto"
    a = build(B, c)
    P, dead = {}, {}
    for name, group, tgt in models(c):
        n = get(a, c, name).size
        in_dim, units, _, oc = nets.get(group, (0, (0,), 0, 0))
        P[name] = X.craft_params(rng, n, in_dim, units[0] if in_dim else 0, oc, X.param_hi(c))
        if c.agent in ("sac", "candle_sac") and group == "actor" and c.shape != "small":
            P[name] = X.thin_hidden_layers(P[name], in_dim, units)
        dead[name] = X.dead_lanes(in_dim, units[0]) if in_dim else None
        if tgt:
            P[tgt] = X.craft_targets(rng, P[name])
    la0 = np.float32([rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])])
    batch = make(c, rng)

    def write(agent, moments=None):
        for k, x in P.items():
            put(agent, c, x, k)
        if auto:
            agent.set_params(la0, "log_alpha")
        for name, st in (moments or {}).items():
            for role, key in (("exp_avg", "m"), ("exp_avg_sq", "v"), ("max_exp_avg_sq", "vmax")):
                if st[key] is not None:
                    (agent.set_params(st[key], name, role) if name == "log_alpha" else put(agent, c, st[key], name, role))

    # the step's gradient, from a second agent (it depends on the parameters and the batch, not on the optimizer's state)
    pa = build(B, c)
    write(pa)
    step(pa, c, batch)
    G0 = {name: get(pa, c, name, "grad") for name, _, _ in models(c)}
    if auto:
        G0["log_alpha"] = (pa.get_params("log_alpha", "grad") if c.agent == "candle_sac"
                           else np.float32([-(np.asarray(pa.probe("log_p", X.BATCH), np.float64).mean() + TARGET_ENTROPY)]))
    pa.close()
    # warm-up: t - 1 updates
    for _ in range(c.t - 1):
        step(a, c, make(c, rng))
    assert a.n_opts == c.t - 1
    M = {}
    for name, group, _ in models(c):
        m, v, vmax = X.craft_moments(rng, G0[name], X.scalars_of(c.opts[group], c.t), ams[group], dead[name])
        M[name] = dict(m=m, v=v, vmax=vmax)
    if auto:
        m, v, _ = X.craft_moments(rng, G0["log_alpha"], X.scalars_of(X.case_configs(c)["log_alpha"], c.t, ENT_LR), False)
        M["log_alpha"] = dict(m=m, v=v, vmax=None)
    write(a, M)
    before = snapshot(a, c, ams)
    for name, group, tgt in models(c):           # set -> get round-trips the bits
        same_bits((c.name, name, "round trip p"), before[name]["p"], P[name])
        same_bits((c.name, name, "round trip m"), before[name]["m"], M[name]["m"])
        same_bits((c.name, name, "round trip v"), before[name]["v"], M[name]["v"])
        if ams[group]:
            same_bits((c.name, name, "round trip vmax"), before[name]["vmax"], M[name]["vmax"])
        if tgt:
            same_bits((c.name, tgt, "round trip"), before[tgt], P[tgt])
    la_before = log_alpha_state(a) if c.agent in ("sac", "candle_sac") else None
    step(a, c, batch)
    after = snapshot(a, c, ams)
    assert a.n_opts == c.t
    live = []
    for name, group, tgt in models(c):
        g = get(a, c, name, "grad")
        assert np.isfinite(g).all(), (c.name, name)
        live.append(float((g != 0).mean()))
        print(c.name, name, "non-zero gradient entries", live[-1], "largest |g|", float(np.abs(g).max()))
        s = X.scalars_of(c.opts[group], c.t)     # this model's own optimizer at this model's own counter
        check_adam((c.name, name), before[name], g, after[name], s)
        if dead[name] is not None:
            da, db = dead[name]
            assert (g[da] == 0).all() and (g[db] == 0).all(), (c.name, name, "a dead lane has a gradient")
            same_bits((c.name, name, "m = v = 0, g = 0: p' = p wd_mul"), after[name]["p"][db], before[name]["p"][db] * s["wd_mul"])
            assert np.isfinite(after[name]["p"][db]).all()
        if tgt:
            check_track((c.name, tgt), after[name]["p"], before[tgt], after[tgt], c.tau)
    assert max(live) > 0.25, (c.name, "no model of the case has a live gradient", live)
    if la_before is not None:
        if auto:
            check_log_alpha(a, c, la_before, c.t)
        else:                                    # Fix(alpha): the update must not touch it
            for k, x in log_alpha_state(a).items():
                same_bits((c.name, "log_alpha kept", k), x, la_before[k])
    # lanes beyond the reference layout stay zero and finite: ten more updates, everything still finite, the forward pass too
    for _ in range(10):
        step(a, c, make(c, rng))
    for name, st in snapshot(a, c, ams).items():
        for k, x in (st.items() if isinstance(st, dict) else [("p", st)]):
            assert x is None or np.isfinite(x).all(), (c.name, name, k, "after ten more updates")
    assert forward_is_finite(a, c, batch), c.name
    assert a.n_opts == c.t + 10
    a.close()


@pytest.mark.parametrize("name", [c.name for c in X.CASES])
def test_optimizer_step_and_soft_update(B, monkeypatch, name):
    run_case(B, X.CASE[name], monkeypatch)


# ------------------------------------------------------------------------------------------------ the soft-update interval
INTERVAL_CASES = ["dqn_mlp_global_adamw_t2", "dqn_mlp_lds_adamw_t1", "dqn_mlp_layers_adam_t10_tau1", "iqn_adam_t1"]


@pytest.mark.parametrize("name", INTERVAL_CASES)
def test_soft_update_interval_three_over_seven_updates(B, monkeypatch, name):
    """soft_update_interval = 3, seven updates: the target's bits change after exactly the updates the reference's counter names (3 and 6),
    there they are track_f32 of the POST-step parameters, and between them the target keeps its bits."""
    c = X.CASE[name]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    tau = 0.5 if c.tau in (0.0, 1.0) else c.tau
    c = X.Case(c.name, c.agent, c.path, c.kernels, c.shape, c.opts, c.t, tau, c.nc, c.env, c.extra)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    a = build(B, c, soft_update_interval=3)
    (model, _, tgt), = models(c)
    p = X.craft_params(rng, get(a, c, model).size, hi=X.param_hi(c))
    put(a, c, p, model)
    put(a, c, X.craft_targets(rng, p), tgt)
    hits = X.track_schedule(3, [1] * 7)
    assert hits == [False, False, True, False, False, True, False]
    t32, o32 = X.tau_scalars(tau)
    for k, hit in enumerate(hits):
        t0 = get(a, c, tgt)
        step(a, c, make(c, rng))
        p1, t1 = get(a, c, model), get(a, c, tgt)
        if hit:
            same_bits((name, "update", k + 1, "tracked from the post-step parameters"), t1, X.track_f32(p1, t0, t32, o32))
            assert (bits(t1) != bits(t0)).mean() > 0.9
        else:
            same_bits((name, "update", k + 1, "between intervals the target keeps its bits"), t1, t0)
    assert a.n_opts == 7
    a.close()


@pytest.mark.parametrize("env", [(), (("BDR_NO_MLP_LDS", "1"),), (("BDR_NO_MLP_FUSED", "1"),)])
def test_soft_update_interval_counts_opts_not_updates(B, monkeypatch, env):
    """n_updates_per_opt = 2 over the replay ring (Agent::opt), soft_update_interval = 3, four opts: the counter ticks once per opt
    (dqn/base.rs:190-198), so the target moves after opt 3 only - not after update 3 - and from the parameters after that opt's SECOND update."""
    c = X.CASE["dqn_mlp_lds_adamw_t1"]
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    od = X.SHAPES[c.shape]["obs"]
    rng = np.random.default_rng(5)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=256, seed=9), (od,), np.float32)
    n = 64
    rb.push(rng.uniform(1, 2, (n, od)).astype(np.float32), rng.integers(0, X.N_ACTIONS, (n, 1)).astype(np.int64), rng.uniform(1, 2, (n, od)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), (rng.random(n) < .1).astype(np.int8), np.zeros(n, np.int8))
    c = X.Case(c.name, c.agent, c.path, c.kernels, c.shape, c.opts, c.t, 0.5, c.nc, env, c.extra)
    a = build(B, c, soft_update_interval=3, n_updates_per_opt=2)
    p = X.craft_params(rng, a.get_params("qnet").size)
    a.set_params(p, "qnet"); a.set_params(X.craft_targets(rng, p), "qnet_tgt")
    t32, o32 = X.tau_scalars(0.5)
    for k, hit in enumerate(X.track_schedule(3, [2] * 4)):
        t0 = a.get_params("qnet_tgt")
        a.opt(rb); a.sync()
        p1, t1 = a.get_params("qnet"), a.get_params("qnet_tgt")
        if hit:
            assert k == 2
            same_bits(("opt", k + 1, "tracked from the parameters after the opt's last update"), t1, X.track_f32(p1, t0, t32, o32))
        else:
            same_bits(("opt", k + 1, "between intervals the target keeps its bits"), t1, t0)
    assert a.n_opts == 4
    a.close(); rb.close()


# ------------------------------------------------------------------------------------------------ SAC: the captured graph and the queues
def _sac_opt_run(B, monkeypatch, env):
    """four opts over the ring from the same seeds: the state before and after each (every model, every role), and the gradients"""
    c = X.Case("sac_graph", "sac", "graph", (), "small", dict(actor=X.ADAMW, critic=X.ADAMW_B), 1, 0.5, 2, extra=(("ent", "auto"),))
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    od, ad, _ = _dims(c)
    rng = np.random.default_rng(17)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=512, seed=7), (od,), np.float32, (ad,), np.float32)
    n = 128
    rb.push(rng.uniform(1, 2, (n, od)).astype(np.float32), rng.uniform(-1, 1, (n, ad)).astype(np.float32), rng.uniform(1, 2, (n, od)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32), (rng.random(n) < .05).astype(np.int8), np.zeros(n, np.int8))
    a = build(B, c)
    a.train()
    ams = dict(actor=False, critic=False)
    for name, group, tgt in models(c):
        p = X.craft_params(rng, get(a, c, name).size, hi=X.param_hi(c))
        put(a, c, p, name)
        if tgt:
            put(a, c, X.craft_targets(rng, p), tgt)
    states, grads = [snapshot(a, c, ams)], []
    la = [log_alpha_state(a)]
    for _ in range(4):
        a.opt(rb); a.sync()
        states.append(snapshot(a, c, ams))
        grads.append({name: get(a, c, name, "grad") for name, _, _ in models(c)})
        la.append(log_alpha_state(a))
    assert a.n_opts == 4
    a.close(); rb.close()
    return c, states, grads, la


def test_sac_captured_graph_steps_1_to_4_carry_their_own_scalars(B, monkeypatch):
    """Agent::opt from the captured graph (its Adam scalars are patched per replay), eagerly on two queues and eagerly on one: at every
    step t = 1..4 each model's state after is adam_f32 / track_f32 of the state before and the read-back gradient AT THAT t - a stale
    patched scalar would show - and the three runs agree bit for bit."""
    runs = {}
    for tag, env in (("graph", (("BDR_STEP_GRAPH", "1"),)), ("eager, two queues", (("BDR_NO_STEP_GRAPH", "1"),)),
                     ("eager, one queue", (("BDR_NO_STEP_GRAPH", "1"), ("BDR_SAC_SIDE_QUEUE", "0")))):
        c, states, grads, la = _sac_opt_run(B, monkeypatch, env)
        runs[tag] = (states, la)
        for t in range(1, 5):
            for name, group, tgt in models(c):
                check_adam((tag, "t", t, name), states[t - 1][name], grads[t - 1][name], states[t][name], X.scalars_of(c.opts[group], t))
                if tgt:
                    check_track((tag, "t", t, tgt), states[t][name]["p"], states[t - 1][tgt], states[t][tgt], c.tau)
    ref_states, ref_la = runs["graph"]
    for tag, (states, la) in runs.items():
        for t in range(5):
            for k in "pmv":
                same_bits((tag, "log_alpha", t, k), la[t][k], ref_la[t][k])
            for name, st in states[t].items():
                for k, x in (st.items() if isinstance(st, dict) else [("p", st)]):
                    if x is not None:
                        same_bits((tag, "t", t, name, k), x, ref_states[t][name][k] if isinstance(st, dict) else ref_states[t][name])
