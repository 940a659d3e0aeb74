"""Construction checks of tests/optimizer_inputs.py (no GPU): the bars hold for the f32 restatement, the restatement agrees with the
form candle-nn documents, every mutation moves a compared quantity by at least 10 bars on a listed case's crafted inputs, the dead
lanes have no gradient in a float64 forward and backward, and the case table covers every kernel and path of DESIGN.md section 16."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimizer_inputs as X  # noqa: E402

RUN = [c for c in X.CASES if not c.refusal]


def configs():
    """every (case, model group, Opt, t) of the table"""
    return [(c, g, o, c.t) for c in RUN for g, o in X.case_configs(c).items()]


def state_of(c, g, o, t, **kw):
    return X.crafted_state(zlib.crc32(f"{c.name}/{g}".encode()), o, t, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_scalars_are_double_arithmetic_cast_once():
    s = X.adam_scalars(True, 1e-2, 0.8, 0.9, 1e-3, 0.1, 1)
    assert s["sqrt_bc2"] == np.float32(np.sqrt(1.0 - 0.9)) and s["neg_step"] == np.float32(-(1e-2 / (1.0 - 0.8))) and s["wd_mul"] == np.float32(1.0 - 1e-3)
    assert abs(float(s["sqrt_bc2"]) ** 2 - 0.1) < 1e-7                                   # t = 1: bc2 = 1 - beta2
    d = X.adam_scalars(False, 1e-2, 0.8, 0.9, 1e-3, 0.1, 1)                             # plain Adam: tch's fixed defaults, whatever is configured
    assert (d["b1"], d["b2"], d["eps"], d["wd_mul"]) == (np.float32(0.9), np.float32(0.999), np.float32(1e-8), np.float32(1.0))
    assert all(v.dtype == np.float32 for v in s.values())


@pytest.mark.parametrize("c,g,o,t", configs(), ids=lambda x: x.name if isinstance(x, X.Case) else None)
def test_f32_restatement_lies_within_the_derived_bars(c, g, o, t):
    st = state_of(c, g, o, t)
    s = X.scalars_of(o, t)
    got = X.adam_f32(st["p"], st["g"], st["m"], st["v"], st["vmax"], s)
    (ref, _), bars = X.adam_f64(st["p"], st["g"], st["m"], st["v"], st["vmax"], s), X.adam_bars(st["p"], st["g"], st["m"], st["v"], st["vmax"], s)
    for k, a, r in zip(("p", "m", "v", "vmax"), got, ref):
        if a is None:
            continue
        assert np.isfinite(a).all() and (bars[k] > 0).all()
        worst = float((np.abs(a.astype(np.float64) - r) / bars[k]).max())
        assert worst <= 1.0, (k, worst)
    t32, o32 = X.tau_scalars(c.tau)
    tr = X.track_f32(got[0], st["tgt"], t32, o32)
    assert (np.abs(tr.astype(np.float64) - X.track_f64(got[0], st["tgt"], t32, o32)) <= X.track_bar(got[0], st["tgt"], t32, o32)).all()


@pytest.mark.parametrize("c,g,o,t", [x for x in configs() if not x[2].amsgrad], ids=lambda x: x.name if isinstance(x, X.Case) else None)
def test_candle_form_agrees_within_the_bar(c, g, o, t):
    """the restatement against the formula candle-nn documents (m_hat = m / bc1, v_hat = v / bc2, p -= lr m_hat / (sqrt(v_hat) + eps) after
    p *= 1 - lr wd), evaluated from the configuration's doubles: within the same bar, element by element (candle-nn's AdamW has no
    amsgrad, so the amsgrad configurations have no such form to be compared with)"""
    st = state_of(c, g, o, t)
    s = X.scalars_of(o, t)
    (ref, _), bars = X.adam_f64(st["p"], st["g"], st["m"], st["v"], None, s), X.adam_bars(st["p"], st["g"], st["m"], st["v"], None, s)
    p1, m1, v1 = X.candle_adamw_f64(st["p"], st["g"], st["m"], st["v"], o, t)
    for k, a, r in (("p", p1, ref[0]), ("m", m1, ref[1]), ("v", v1, ref[2])):
        worst = float((np.abs(a - r) / bars[k]).max())
        assert worst <= 1.0, (k, worst)


@pytest.mark.parametrize("mutation", list(X.MUTATIONS))
def test_every_mutation_moves_a_compared_quantity_by_ten_bars(mutation):
    """DESIGN.md section 12's rule: a case that cannot tell a wrong kernel from a right one does not pass"""
    assert mutation in X.CATCHES and X.CATCHES[mutation]
    moved = {}
    for name in X.CATCHES[mutation]:
        c = X.CASE[name]
        assert not c.refusal
        best = 0.0
        for g, o in X.case_configs(c).items():
            st = state_of(c, g, o, c.t)
            if mutation == "cross_model_t":
                # every counter of an agent advances once per update, so on the device the counters are equal and this mutation shows only
                # as a wrong step number of the model itself (t_minus_1 / t_plus_1); restated here with the neighbour one update ahead
                st["t_other"] = c.t + 1
            best = max(best, X.sensitivity(mutation, o, c.t, c.tau if c.tau not in (0.0, 1.0) else 0.5, st))
        moved[name] = best
    print(mutation, moved)
    assert max(moved.values()) >= 10.0, moved


def test_listed_t_mutations_hold_in_every_listed_case():
    """a step counter off by one is caught by EVERY case that lists it, not just by one of them (t = 1000 included: 1 - 0.999^t still moves)"""
    for mutation in ("t_minus_1", "t_plus_1"):
        for name in X.CATCHES[mutation]:
            c = X.CASE[name]
            best = max(X.sensitivity(mutation, o, c.t, 0.5, state_of(c, g, o, c.t)) for g, o in X.case_configs(c).items())
            assert best >= 10.0, (mutation, name, best)


@pytest.mark.parametrize("c", [c for c in RUN if X.model_nets(c)], ids=lambda c: c.name)
def test_dead_lanes_have_no_gradient_in_float64(c):
    """a float64 forward and backward of the case's network on the case's rows - and on the corners a policy's action can reach: the
    gradient of the dead units' incoming weights and biases is exactly 0, whatever gradient arrives from above"""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    sh = X.SHAPES[c.shape]
    b = X.make_batch(rng, X.BATCH, sh["obs"], sh["act"])
    for group, (in_dim, units, out_dim, oc) in X.model_nets(c).items():
        n = sum(a * b_ + a for a, b_ in zip(list(units) + [out_dim], [in_dim] + list(units)))
        p = X.craft_params(rng, n, in_dim, units[0], oc, X.param_hi(c))
        assert (np.abs(p) >= 0.5).all() and (np.abs(p) <= 8.0).all()
        rows = [np.concatenate([b["obs"], b["act"]], 1)[:, :in_dim] if in_dim > oc else b["obs"]]
        if in_dim > oc:   # the action columns at +1 and -1: a tanh or a clamp cannot leave that box
            rows += [np.concatenate([b["next_obs"], np.full((X.BATCH, in_dim - oc), s, np.float32)], 1) for s in (1.0, -1.0)]
        g = dead_g = X.dead_gradient_f64(in_dim, units, out_dim, p, np.concatenate(rows), seed=1)
        da, db = X.dead_lanes(in_dim, units[0])
        assert (dead_g[da] == 0).all() and (dead_g[db] == 0).all(), (c.name, group)
        assert (g != 0).mean() > 0.2                     # ... and the live units do have one


def test_dead_lane_updates_are_what_only_eps_and_the_decay_decide():
    for o, t in ((X.ADAMW, 1), (X.ADAM, 2), (X.ADAMW_B, 10)):
        st = X.crafted_state(11, o, t)
        s = X.scalars_of(o, t)
        p1, m1, v1, _ = X.adam_f32(st["p"], st["g"], st["m"], st["v"], None, s)
        da, db = st["dead"]
        assert (st["g"][da] == 0).all() and (st["m"][da] == np.float32(1e-9)).all() and (st["v"][da] == 0).all() and (st["m"][db] == 0).all()
        assert (bits(p1[db]) == bits(st["p"][db] * s["wd_mul"])).all() and np.isfinite(p1[db]).all()          # m = v = 0: p' = p wd_mul, bit for bit
        want = st["p"][da] * s["wd_mul"] + s["neg_step"] * (np.float32(1e-9) * s["b1"]) / (np.float32(0) / s["sqrt_bc2"] + s["eps"])
        assert (bits(p1[da]) == bits(want)).all() and np.isfinite(p1[da]).all()                              # m = 1e-9, v = 0: neg_step b1 m / eps
        if not o.adamw:   # under plain Adam nothing but eps sets that step's size: another eps, another step, by far more than the bar
            assert X.sensitivity("eps_in_sqrt", o, t, 0.5, st) >= 10.0


def test_crafted_state_is_what_the_cases_ask_for():
    o, t = X.AMSGRAD, 2
    st = X.crafted_state(5, o, t, n=3000)
    p, g, m, v, vmax = (st[k].astype(np.float64) for k in ("p", "g", "m", "v", "vmax"))
    live = g != 0
    assert (np.abs(p) >= 0.5).all() and (np.abs(p) <= 8).all()
    assert 0.3 < (np.sign(m[live]) == -np.sign(g[live])).mean() < 0.7            # exp_avg opposes g on about half the entries
    i = np.arange(g.size)
    assert (v[i % 3 == 0] == 0).all()
    r = v[live & (i % 3 == 1)] / g[live & (i % 3 == 1)] ** 2
    assert (r > 0.4).all() and (r < 2.1).all()
    r = v[live & (i % 3 == 2)] / g[live & (i % 3 == 2)] ** 2
    assert np.allclose(r, 1e4, rtol=1e-5)
    s = X.scalars_of(o, t)
    v1 = X.adam_f32(st["p"], st["g"], st["m"], st["v"], st["vmax"], s)[2].astype(np.float64)
    pos = v1 > 1e-30
    assert 0.4 < (vmax[pos] > v1[pos]).mean() < 0.6 and 0.4 < (vmax[pos] < v1[pos]).mean() < 0.6
    tg = st["tgt"].astype(np.float64) - p
    assert (tg >= 0.49).all() and (tg <= 1.51).all()


def test_thinned_actor_trunks_keep_the_range_the_dead_lanes_and_four_live_units_per_layer():
    import torch
    rng = np.random.default_rng(9)
    for shape in ("ragged", "deep"):
        sh = X.SHAPES[shape]
        od, units = sh["obs"], sh["units"]
        n = sum(a * b + a for a, b in zip(units, (od,) + tuple(units)))
        p0 = X.craft_params(rng, n, od, units[0], od, 0.75)
        p = X.thin_hidden_layers(p0, od, units)
        assert (np.abs(p) == np.abs(p0)).all() and (np.abs(p) >= 0.5).all()
        x = torch.tensor(rng.uniform(X.OBS_LO, X.OBS_HI, (64, od)))
        o, i = 0, od
        for l, u in enumerate(units):
            W, b = torch.tensor(p[o:o + u * i].reshape(u, i), dtype=torch.float64), torch.tensor(p[o + u * i:o + u * i + u], dtype=torch.float64)
            x = torch.relu(x @ W.T + b)
            first = (X.N_DEAD if l == 0 else 0) + X.K_LIVE
            assert (x[:, first:] == 0).all() and (l > 0 or (x[:, :X.N_DEAD] == 0).all())
            o, i = o + u * i + u, u
        assert float(x.abs().max()) * 0.75 * X.K_LIVE + 0.75 < 88.0          # the heads' pre-activations stay where exp() is finite


def test_the_root_one_ulp_off_stays_within_the_bar_and_rarely_shows_in_p():
    """the hardware root's allowance (adam_f32, sqrt_ulps): one ulp of the root is inside p's bar, moves few elements, and never exp_avg or exp_avg_sq"""
    o, t = X.ADAMW, 2
    st = X.crafted_state(21, o, t, n=3000)
    s = X.scalars_of(o, t)
    args = (st["p"], st["g"], st["m"], st["v"], None, s)
    base, (ref, _), bars = X.adam_f32(*args), X.adam_f64(*args), X.adam_bars(*args)
    for u in (-1, 1):
        got = X.adam_f32(*args, sqrt_ulps=u)
        assert (bits(got[1]) == bits(base[1])).all() and (bits(got[2]) == bits(base[2])).all()
        assert (np.abs(got[0].astype(np.float64) - ref[0]) <= bars["p"]).all()
        assert (bits(got[0]) != bits(base[0])).mean() < 0.1
    forms = {f: X.log_alpha_step_f32(st["p"], st["g"], st["m"], st["v"], s, f) for f in X.LOG_ALPHA_FORMS}
    plain = X.adam_f32(st["p"], st["g"], st["m"], st["v"], None, dict(s, wd_mul=np.float32(1.0)))
    assert all((bits(forms[("", "", 0)][k]) == bits(plain[k])).all() for k in range(3))      # unfused, rounded root: adam_element without decay
    for f, got in forms.items():                                                                # a fused product saves a rounding: still inside the bars
        b1 = X.adam_bars(st["p"], st["g"], st["m"], st["v"], None, dict(s, wd_mul=np.float32(1.0)))
        r1 = X.adam_f64(st["p"], st["g"], st["m"], st["v"], None, dict(s, wd_mul=np.float32(1.0)))[0]
        assert all((np.abs(got[k].astype(np.float64) - r1[k]) <= b1[key]).all() for k, key in enumerate("pmv")), f


def test_tau_one_and_zero_in_the_restatement():
    rng = np.random.default_rng(2)
    src, dst = X.craft_params(rng, 500), X.craft_params(rng, 500)
    assert (bits(X.track_f32(src, dst, *X.tau_scalars(1.0))) == bits(src)).all()
    assert (bits(X.track_f32(src, dst, *X.tau_scalars(0.0))) == bits(dst)).all()
    t32, o32 = X.tau_scalars(0.005)
    assert t32 == np.float32(0.005) and o32 == np.float32(0.995)


def test_track_schedule_is_the_reference_counter():
    assert X.track_schedule(3, [1] * 7) == [False, False, True, False, False, True, False]
    assert X.track_schedule(3, [1, 2, 1, 1]) == [False, False, True, False]      # one tick per opt, whatever n_updates_per_opt is
    assert X.track_schedule(1, [1] * 3) == [True] * 3


def test_the_table_covers_every_kernel_path_step_and_rate():
    named = {k for c in RUN for k in c.kernels}
    for k in ("k_adam", "k_adam_amsgrad", "k_track", "mlp_fused.hpp LDS step", "mlp_fused.hpp global step", "k_reduce_adam vector body",
              "k_reduce_adam segment body", "k_dense_reduce_adam", "log-alpha (k_sac_select)", "log-alpha (k_sac_q_last / tail)", "log-alpha (k_csac_alpha)"):
        assert k in named, k
    agents = {c.agent for c in RUN}
    assert agents == {"sac", "candle_sac", "iql", "awac", "bc", "dqn_mlp", "dqn_cnn", "iqn"}
    assert {c.t for c in RUN} == set(X.TS) and {c.tau for c in RUN if c.agent != "bc"} == set(X.TAUS)
    assert {c.shape for c in RUN} == set(X.SHAPES)
    assert {c.nc for c in X.CASES if c.agent in ("sac", "candle_sac", "iql", "awac")} == {1, 2, 4, 5}
    assert all(c.refusal for c in X.CASES if c.nc == 5)                        # RA_INST = 4 is the constructors' limit: five critics are refused
    assert {c.x("form") for c in RUN if c.agent == "bc"} == {"general", "fused", "fused_mfma"}
    assert {c.x("actor") for c in RUN if c.agent == "candle_sac"} == {"Mlp2", "Mlp3"}
    paths = {(c.agent, c.path) for c in RUN}
    for p in (("dqn_mlp", "LDS step"), ("dqn_mlp", "BDR_NO_MLP_LDS"), ("dqn_mlp", "BDR_NO_MLP_FUSED"), ("sac", "row-block"), ("sac", "BDR_NO_SAC_FUSE"),
              ("iqn", "plain"), ("iqn", "amsgrad")):
        assert p in paths, p
    for c in RUN:   # amsgrad on DQN, IQN and the tch SAC's critics only
        for g, o in c.opts.items():
            assert not o.amsgrad or (c.agent in ("dqn_mlp", "dqn_cnn", "iqn") or (c.agent == "sac" and g == "critic"))
    for name, cases in X.CATCHES.items():
        assert name in X.MUTATIONS and all(n in X.CASE for n in cases)
    assert set(X.CATCHES) == set(X.MUTATIONS)
