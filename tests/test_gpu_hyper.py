"""Hyperparameters by id (bdr_agent_hyper_get / _set through Bc / Iql / Awac / CandleSac .get_hyper / .set_hyper and the groups' forms):
a value set before the first update equals one given at creation, bit for bit over every (model, role) of the parameter views, for
every id of every kind, standalone and as a group member; a set in the middle of a run reaches a group's staged arguments as it reaches
the standalone agent; BC's learning rate switched in mid-run follows tests/bc_restatement.py driven with the same switch.
tests/group_copy_cases.py has the kinds' configs (every optimizer AdamW, so that betas, eps and weight decay are read) and state."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bc_restatement as R  # noqa: E402
import group_copy_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = tuple(K.SHAPES)
UPDATES = 3


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def shape_of(kind):
    return K.SHAPES[kind]["partial_block"]


def build(B, kind, h, seed=3):
    return getattr(B, K.AGENTS[kind]).build(K.config(B, kind, shape_of(kind), h, seed))


@pytest.mark.parametrize("kind", KINDS)
def test_set_before_the_first_update_equals_given_at_creation_standalone(B, kind):
    shape = shape_of(kind)
    y = K.hypers(kind, 1, shape[1])
    owner = K.dataset(B, shape)
    for name in K.hyper_names(kind):
        x = dict(y, **{name: K.other_value(name, y[name])})
        made, set_ = build(B, kind, x), build(B, kind, y)
        assert set_.get_hyper(name) == y[name]
        set_.set_hyper(name, x[name])
        assert set_.get_hyper(name) == x[name] == made.get_hyper(name)
        views = [owner.view(50), owner.view(50)]
        for _ in range(UPDATES):
            made.opt(views[0]); set_.opt(views[1])
        K.assert_same(K.state(kind, set_), K.state(kind, made), name)
        for a in (made, set_):
            a.close()
        for v in views:
            v.close()
    owner.close()


@pytest.mark.parametrize("kind", KINDS)
def test_set_before_the_first_round_equals_given_at_creation_as_a_group_member(B, kind):
    """one group: for every id a member built with y and set to x before the first round, beside a member built with x"""
    shape = shape_of(kind)
    y = K.hypers(kind, 1, shape[1])
    names = K.hyper_names(kind)
    xs = [dict(y, **{n: K.other_value(n, y[n])}) for n in names]
    cfgs = [c for x in xs for c in (K.config(B, kind, shape, y, 3), K.config(B, kind, shape, x, 3))]
    g = getattr(B, K.GROUPS[kind]).build(cfgs + [K.config(B, kind, shape, y, 3)])   # the last member stays at y
    for k, n in enumerate(names):
        g.set_hyper(2 * k, n, xs[k][n])
        assert g.get_hyper(2 * k, n) == xs[k][n] == g.get_hyper(2 * k + 1, n)
    owner = K.dataset(B, shape)
    views = [owner.view(50) for _ in range(len(g))]
    for _ in range(UPDATES):
        g.opt(views)
    g.sync()
    left = K.state(kind, g.members[-1])
    for k, n in enumerate(names):
        s = K.state(kind, g.members[2 * k])
        K.assert_same(s, K.state(kind, g.members[2 * k + 1]), n)
        if n != "exp_adv_max":   # (a clamp that binds for large advantages only: three updates from the initial networks need not reach it)
            assert not K.same(s, left), n   # the value is read: the member left at y has gone elsewhere
    g.close()
    for v in views:
        v.close()
    owner.close()


@pytest.mark.parametrize("kind", KINDS)
def test_setting_a_value_to_what_it_is_changes_no_bit(B, kind):
    shape = shape_of(kind)
    h = K.hypers(kind, 1, shape[1])
    g = getattr(B, K.GROUPS[kind]).build([K.config(B, kind, shape, h, 3) for _ in range(2)])
    owner = K.dataset(B, shape)
    views = [owner.view(50), owner.view(50)]
    for _ in range(UPDATES):
        g.opt(views)
        for n in h:
            g.set_hyper(0, n, g.get_hyper(0, n))
            assert g.get_hyper(0, n) == h[n]
    g.sync()
    K.assert_same(K.state(kind, g.members[0]), K.state(kind, g.members[1]), kind)
    g.close()
    for v in views:
        v.close()
    owner.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_set_in_mid_run_reaches_the_group_as_it_reaches_the_agent(B, kind):
    """two rounds, every hyperparameter of member 1 set to another value, two more rounds: the group (whose staged arguments hold gamma,
    the taus, inv_lambda, exp_adv_max and the target entropy) against the same agents stepped alone with the same sets"""
    shape = shape_of(kind)
    hs = [K.hypers(kind, i, shape[1]) for i in range(2)]
    owner = K.dataset(B, shape)
    out = []
    for grouped in (True, False):
        agents = [build(B, kind, hs[i], 3 + i) for i in range(2)]
        views = [owner.view(50 + i) for i in range(2)]
        g = getattr(B, K.GROUPS[kind])(agents) if grouped else None
        for k in range(4):
            if k == 2:
                for n, v in hs[1].items():
                    agents[1].set_hyper(n, K.other_value(n, v))
            if grouped:
                g.opt(views)
            else:
                for a, v in zip(agents, views):
                    a.opt(v)
        for a in agents:
            a.sync()
        out.append([K.state(kind, a) for a in agents])
        if grouped:
            g.close()
        else:
            for a in agents:
                a.close()
        for v in views:
            v.close()
    owner.close()
    for i in range(2):
        K.assert_same(out[0][i], out[1][i], i)


@pytest.mark.parametrize("kind", KINDS)
def test_unknown_ids_and_values_out_of_range_are_refused(B, kind):
    shape = shape_of(kind)
    h = K.hypers(kind, 0, shape[1])
    a = build(B, kind, h)
    missing = {"bc": ("gamma", "lr_actor", 5, 99, -1), "iql": ("lr", "ent_coef_lr", 35, 47), "awac": ("lr", "tau_iql", "lr_value", 15),
               "candle_sac": ("lr", "inv_lambda", "lr_value", 25)}[kind]
    for name in missing:
        for call in (lambda: a.get_hyper(name), lambda: a.set_hyper(name, 0.5)):
            with pytest.raises(B.BdrError, match="no hyperparameter") as e:
                call()
            assert e.value.code == 1   # BDR_ERR_INVALID
    bad = {n: (-1e-3, float("nan"), float("inf")) for n in h if n.startswith("lr") or n.endswith("eps") or n.endswith("weight_decay") or n == "ent_coef_lr"}
    bad.update({n: (1.0, -0.1, float("nan")) for n in h if n.endswith("beta1") or n.endswith("beta2")})
    bad.update({n: (1.5, -0.1, float("nan")) for n in h if n in ("gamma", "critic_tau")})
    bad.update({"tau_iql": (0.0, 1.0, float("nan")), "inv_lambda": (-1.0, float("inf")), "exp_adv_max": (-1.0, float("nan")), "target_entropy": (float("nan"), float("-inf"))})
    for n in h:
        for v in bad[n]:
            with pytest.raises(B.BdrError) as e:
                a.set_hyper(n, v)
            assert e.value.code == 1, (n, v)
            assert a.get_hyper(n) == h[n], (n, v)
    a.close()
    if kind == "candle_sac":   # the entropy learning rate and target exist with EntCoefMode::Auto only
        fix = build(B, kind, K.hypers(kind, 0, shape[1], auto=False))
        for n in ("ent_coef_lr", "target_entropy"):
            with pytest.raises(B.BdrError, match="no hyperparameter"):
                fix.set_hyper(n, 0.1)
        fix.close()


@pytest.mark.parametrize("form", ("general", "fused_mfma"))
def test_bc_learning_rate_switched_in_mid_run_against_the_restatement(B, form):
    """two updates at learning rate a, two at b, the restatement's optimizer switched at the same update.  The tolerances are those
    tests/test_gpu_bc.py holds a free run of five updates to - the loss within 5e-4 |want| + 1e-6, pred and dz within 1e-4 relative,
    the gradient within 2e-3 relative, the parameters within 0.3 lr - with lr the smaller of the two rates for every update."""
    lr_a, lr_b = 1e-3, 2.5e-3
    spec = R.BcSpec(45, 24, (256, 256), "Tanh", lr=lr_a, adamw=dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01))
    bsz, seed = 256, 11
    params = spec.init_params(seed)
    a = B.Bc.build(spec.to_config(B, bsz, device=0, kernel_form=form))
    a.set_params(params)
    ref = R.BcRestatement(spec, params)

    def rel(x, want):
        x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
        return np.abs(x - want).max() / max(np.abs(want).max(), 1e-30)
    for s in range(4):
        if s == 2:
            a.set_hyper("lr", lr_b)
            ref.opt.lr = lr_b
        batch = R.make_batch(spec, bsz, seed * 100 + s)
        rec, want = a.update_on_batch(*batch), ref.update(*batch)
        figs = (rel(a.probe("pred", bsz), ref.probes["pred"]), rel(a.probe("dz", bsz), ref.probes["dz"]), rel(a.get_params(role="grad"), ref.probes["grad"]),
                np.abs(a.get_params() - ref.params()).max() / min(lr_a, lr_b))
        print(form, s, "loss", rec["loss"], "want", want["loss"], "pred rel %.3g  dz rel %.3g  grad rel %.3g  param step / lr %.3g" % figs)
        assert abs(rec["loss"] - want["loss"]) <= 5e-4 * abs(want["loss"]) + 1e-6, (s, rec, want)
        assert figs[0] < 1e-4 and figs[1] < 1e-4 and figs[2] < 2e-3 and figs[3] < 0.3, (s, figs)
    assert a.get_hyper("lr") == lr_b and a.n_opts == 4
    # and the switch is seen: a twin left at lr_a ends elsewhere
    twin = B.Bc.build(spec.to_config(B, bsz, device=0, kernel_form=form))
    twin.set_params(params)
    for s in range(4):
        twin.update_on_batch(*R.make_batch(spec, bsz, seed * 100 + s))
    assert not np.array_equal(twin.get_params(), a.get_params())
    a.close(); twin.close()
