"""CPU checks of tests/edge_inputs.py: the float64 references are pinned to the committed f32 restatements on ordinary inputs, the dial
networks are bit-exact, every case meets its coverage condition, the committed f32 restatement passes every bar, and every listed
mutation of the reference (a plausible wrong kernel) moves some compared quantity by at least 10 times its bar."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import awac_restatement as RA  # noqa: E402
import bc_restatement as RB  # noqa: E402
import edge_inputs as E  # noqa: E402
import iql_restatement as RI  # noqa: E402

ALL = [(agent, c.name) for agent in E.CASES for c in E.CASES[agent]()]
TEETH = [(agent, c.name, m) for agent in E.CASES for c in E.CASES[agent]() for m in c.muts]


@functools.lru_cache(maxsize=None)
def _case(agent, name):
    case = next(c for c in E.CASES[agent]() if c.name == name)
    ref = E.run_ref(case, terms=True)
    f32out = E.run_f32(case)
    return case, ref, f32out, E.checks_for(case, ref, f32out)


def _close(x, want):
    return abs(x - want) <= 5e-4 * abs(want) + 1e-6


# ---------------------------------------------------------------------------------------------------------- the references are pinned
@pytest.mark.parametrize("extra", [{}, {"critic_loss": "SmoothL1", "action_limit": "Tanh", "action_scale": 2.0},
                                   {"adv_softmax": True, "v_relu_out": True, "q_relu_out": True}])
def test_iql_float64_reference_agrees_with_the_f32_restatement_on_ordinary_inputs(extra):
    """the inputs of tests/test_gpu_iql.py (make_batch, init_params), three free-running steps, at that file's bars"""
    spec = RI.IqlSpec(17, 6, (64, 48), (48, 64), (64, 48), n_critics=2, **extra)
    params = spec.init_params(5)
    batches = [RI.make_batch(spec, 64, 500 + s) for s in range(3)]
    ref = E.IqlRef(spec, *params)
    for b in batches:
        r = ref.update(*b)
    f = E.iql_f32(spec, params, batches)
    for k in ("loss_value", "loss_critic", "loss_actor"):
        assert _close(f[k], float(r[k])), k
    for k in ("q_tgt_min_value", "v", "tgt", "v_next", "q_tgt_min_actor", "v_obs", "logp", "q_pred"):
        assert E.relmax(f[k], r[k]) < 1e-4, k
    assert E.relmax(f["w"], r["w"]) < 2e-3
    for k in ("grad_value", "grad_actor", "grad_critic_0", "grad_critic_1"):
        assert E.relmax(f[k], r[k]) < 2e-3, k
    for k, lr in (("param_value", spec.lr_value), ("param_actor", spec.lr_actor), ("param_critic_1", spec.lr_critic)):
        assert np.abs(f[k] - r[k]).max() < 0.3 * lr, k
    assert E.relmax(f["param_critic_tgt_0"], r["param_critic_tgt_0"]) < 1e-5


@pytest.mark.parametrize("extra,train", [({}, False), ({"critic_loss": "SmoothL1", "action_limit": "Tanh", "action_scale": 2.0}, True),
                                         ({"adv_softmax": True, "q_relu_out": True}, True)])
def test_awac_float64_reference_agrees_with_the_f32_restatement_on_ordinary_inputs(extra, train):
    spec = RA.AwacSpec(17, 6, (64, 48), (48, 64), n_critics=2, **extra)
    params = spec.init_params(5)
    batches = [RA.make_batch(spec, 64, 500 + s) + (spec.draws(64, 550 + s) if train else (None, None)) for s in range(3)]
    ref = E.AwacRef(spec, *params)
    for b in batches:
        r = ref.update(*b)
    f = E.awac_f32(spec, params, batches)
    for k in RA.RECORD_KEYS:
        if k.startswith("adv"):
            assert abs(f[k] - float(r[k])) <= 1e-4 * max(1.0, float(r["q_tgt_abs_mean"])) + 5e-4 * abs(float(r[k])), k
        else:
            assert _close(f[k], float(r[k])), k
    for k in ("q_data_min", "q_pi_min", "next_q", "tgt", "logp", "act_", "next_act", "q_pred"):
        assert E.relmax(f[k], r[k]) < 1e-4, k
    assert E.relmax(f["w"], r["w"]) < 2e-3
    for k in ("grad_actor", "grad_critic_0", "grad_critic_1"):
        assert E.relmax(f[k], r[k]) < 2e-3, k
    assert np.abs(f["param_actor"] - r["param_actor"]).max() < 0.3 * spec.lr_actor
    assert E.relmax(f["param_critic_tgt_1"], r["param_critic_tgt_1"]) < 1e-5


@pytest.mark.parametrize("act_out", ["None", "ReLU", "Tanh", "Sigmoid"])
def test_bc_float64_reference_agrees_with_the_f32_restatement_on_ordinary_inputs(act_out):
    spec = RB.BcSpec(17, 6, (64, 48), act_out)
    params = spec.init_params(5)
    batches = [RB.make_batch(spec, 64, 500 + s) for s in range(3)]
    ref = E.BcRef(spec, params)
    for b in batches:
        r = ref.update(*b)
    f = E.bc_f32(spec, (params,), batches)
    assert _close(f["loss"], r["loss"])
    assert E.relmax(f["pred"], r["pred"]) < 1e-4 and E.relmax(f["dz"], r["dz"]) < 1e-4
    assert E.relmax(f["grad"], r["grad"]) < 2e-3
    assert np.abs(f["param"] - r["param"]).max() < 0.3 * spec.lr


def test_sac_float64_reference_agrees_with_torch_sac_on_ordinary_inputs():
    """the inputs of tests/test_gpu_sac.py's ragged case (init_params * 0.5, sac_batch), two free-running steps, at that file's bars"""
    from oracle import torch_ref as T
    od, ad, pu, qu, nc = 11, 3, (96, 40), (72, 136), 3
    spec = E.SacSpec(od, ad, pu, qu, nc, lr_actor=1e-3, lr_critic=2e-3, ent_coef=("Auto", -3.0, 1e-3), critic_loss="SmoothL1")
    pi0 = T.init_params(T.sac_pi_shapes(od, list(pu), ad), 31) * np.float32(0.5)
    q0 = [T.init_params(T.sac_q_shapes(od, ad, list(qu)), 40 + i) for i in range(nc)]
    batches = [T.sac_batch(72, od, ad, 500 + s) for s in range(2)]
    ref = E.SacRef(spec, pi0, q0, q0)
    for b in batches:
        r = ref.update(*b)
    f = E.sac_f32(spec, (pi0, q0, q0), batches)
    for k in ("loss_critic", "loss_actor", "ent_coef"):
        assert _close(float(f[k]), float(r[k])), k
    for k in ("log_p", "tgt", "q_pred", "grad_pi", "grad_q_0", "grad_q_2"):
        assert E.relmax(f[k], r[k]) < (2e-3 if k.startswith("grad") else 1e-4), k
    assert np.abs(f["param_pi"] - r["param_pi"]).max() < 0.3 * spec.lr_actor
    assert np.abs(f["param_q_1"] - r["param_q_1"]).max() < 0.3 * spec.lr_critic
    assert abs(f["log_alpha"] - float(r["log_alpha"])) < 1e-6


@pytest.mark.parametrize("weighted", [False, True])
def test_dqn_float64_reference_agrees_with_torch_dqn_on_ordinary_inputs(weighted):
    """CartPole-shaped inputs as in tests/test_gpu_dqn.py / test_gpu_per.py, three free-running steps; gradients per variable at 2e-4"""
    from oracle import torch_ref as T
    spec = E.DqnSpec("mlp", 2, in_dim=4, units=(64, 64), gamma=0.99, double_dqn=True, clip_td_err=(0.05, 0.9) if weighted else None)
    p0 = T.init_params(spec.shapes(), 23)
    batches = []
    for s_ in range(3):
        rng = np.random.default_rng(300 + s_)
        b = (rng.standard_normal((32, 4)).astype(np.float32), rng.integers(0, 2, 32), rng.standard_normal((32, 4)).astype(np.float32),
             rng.uniform(-2, 2, 32).astype(np.float32), (rng.random(32) < 0.1).astype(np.int8))
        batches.append(b + ((rng.uniform(0.1, 1.0, 32).astype(np.float32),) if weighted else ()))
    ref = E.DqnRef(spec, p0, p0)
    for b in batches:
        r = ref.update(*b)
    f = E.dqn_f32(spec, (p0, p0), batches)
    assert abs(f["loss"] - float(r["loss"])) <= 1e-4 * abs(float(r["loss"])) + 1e-9
    for k in ("q_pred_all", "q_next_all", "pred", "tgt") + (("td_errs",) if weighted else ()):
        assert E.relmax(f[k], r[k]) < 1e-4, k
    o = 0
    for sh in spec.shapes():
        cnt = int(np.prod(sh))
        assert E.relmax(f["grad"][o:o + cnt], r["grad"][o:o + cnt]) < 2e-4, sh
        o += cnt
    assert np.abs(f["param"] - r["param"]).max() < 0.3 * spec.lr and E.relmax(f["param_tgt"], r["param_tgt"]) < 1e-3


def test_iqn_float64_reference_agrees_with_torch_iqn_on_ordinary_inputs():
    """iqn_batch and init_params as in tests/test_gpu_iqn.py, a small Mlp feature net, three free-running steps"""
    from oracle import torch_ref as T
    spec = E.IqnSpec()
    p0 = T.init_params(spec.shapes(), 31)
    batches = [T.iqn_batch(16, "mlp", spec.n_actions, 8, 8, 70 + s_, in_dim=spec.in_dim) for s_ in range(3)]
    ref = E.IqnRef(spec, p0, p0)
    for b in batches:
        r = ref.update(*b)
    f = E.iqn_f32(spec, (p0, p0), batches)
    assert abs(f["loss_critic"] - float(r["loss_critic"])) <= 1e-4 * abs(float(r["loss_critic"])) + 1e-9
    assert E.relmax(f["z_pred"], r["z_pred"]) < 1e-4 and E.relmax(f["z_tgt"], r["z_tgt"]) < 1e-4
    assert E.relmax(f["grad"], r["grad"]) < 5e-4 and (r["grad"] != 0).mean() > 0.5      # a dense backward
    assert np.abs(f["param"] - r["param"]).max() < 0.1 * spec.lr and E.relmax(f["param_tgt"], r["param_tgt"]) < 1e-5


# ---------------------------------------------------------------------------------------------------------- dial networks
@pytest.mark.parametrize("in_dim,units,out_dim,cols,gain", [
    (9, (32, 48), 1, [4], 1.0),                                   # the shape of the first check of the construction
    (E.IQL_O, (32,), 1, [0], 1.0), (E.IQL_O, (32, 48), E.IQL_A, [5, 6, 7, 8, 9], 1.0), (E.IQL_O + E.IQL_A, (48, 32), 1, [3], 1.0),
    (E.AWAC_O, (32, 48), E.AWAC_A, [0, 1, 2, 3, 4], 1.0), (E.AWAC_O + E.AWAC_A, (48, 32), 1, [E.AWAC_O + 1], 64.0),
    (E.AWAC_O + E.AWAC_A, (48, 32), 1, [E.AWAC_O], 4.0),
    (E.BC_O, (32, 48), E.BC_A, [0, 1, 2, 3, 4], 1.0), (E.BC_O, (64,), E.BC_A, [0, 1, 2, 3, 4], 1.0), (7, (), 3, [6, 0, 2], 1.0),
    (E.SAC_O, (64, 48), 2 * E.SAC_A, list(range(2 * E.SAC_A)), 1.0), (E.SAC_O, (256, 64), 2 * E.SAC_A, list(range(2 * E.SAC_A)), 1.0),   # SAC actor: means | head2
    (2 * E.DQN_A + 2, (64, 64), E.DQN_A, [0, 1, 2], 1.0), (2 * E.DQN_A + 2, (64, 64), E.DQN_A, [3, 4, 5], 1.0),                           # DQN online / target
])
@pytest.mark.parametrize("fill", [False, True])
def test_dial_networks_are_bit_exact_in_the_f32_restatement(in_dim, units, out_dim, cols, gain, fill):
    rng = np.random.default_rng(3)
    flat = E.dial_mlp(in_dim, units, out_dim, cols, gain=gain, rng=np.random.default_rng(1) if fill else None)
    x = rng.standard_normal((64, in_dim)).astype(np.float32)
    x[:7, cols[0]] = E.Z_GRID.astype(np.float32)
    x[7, cols[0]] = np.float32(E.CLAMP1)
    with torch.no_grad():
        y = RI.Mlp(in_dim, units, out_dim, False, flat).forward(torch.as_tensor(x)).numpy()
    assert y.dtype == np.float32
    assert (y == np.float32(gain) * x[:, cols]).all()


@pytest.mark.parametrize("units", [(48, 32), (256, 64)])
def test_two_term_dial_of_the_sac_critics_is_exact_where_one_term_is_zero(units):
    """Q(o, a) = o[8] + gain a[0]: bit-exact on rows where the action column is 0 (the batch actions) and where the state column is 0"""
    rng = np.random.default_rng(4)
    in_dim = E.SAC_O + E.SAC_A
    flat = E.dial_mlp(in_dim, units, 1, [[(8, 1.0), (E.SAC_O, 4.0)]], rng=np.random.default_rng(2))
    x = rng.standard_normal((64, in_dim)).astype(np.float32)
    x[:32, E.SAC_O] = 0.0
    x[32:, 8] = 0.0
    with torch.no_grad():
        y = RI.Mlp(in_dim, units, 1, False, flat).forward(torch.as_tensor(x)).numpy()[:, 0]
    assert (y[:32] == x[:32, 8]).all() and (y[32:] == np.float32(4.0) * x[32:, E.SAC_O]).all()


def test_the_sac_actor_of_a_case_dials_its_mean_and_head2_columns_bit_for_bit():
    """the flat actor of sac_case (the dial's last layer re-split into the ml / sl heads) through oracle.torch_ref.TorchSac.pi_forward"""
    from oracle import torch_ref as T
    case = next(c for c in E.sac_cases() if c.name == "fix_alpha_eps_default")
    s = case.spec
    sac = T.TorchSac(s.obs_dim, s.act_dim, list(s.pi_units), list(s.q_units), case.params[0], case.params[1], lr_actor=0, lr_critic=0)
    obs = torch.as_tensor(case.batches[0][0])
    with torch.no_grad():
        mean, e = sac.pi_forward(obs)
    assert (mean.numpy() == case.batches[0][0][:, :4]).all()
    assert (e.numpy() == torch.as_tensor(case.batches[0][0][:, 4:8]).exp().numpy()).all()     # Mlp2 returns exp(head2)


# ---------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("agent,name", ALL)
def test_case_meets_its_coverage_condition(agent, name):
    case, ref, _, _ = _case(agent, name)
    cov = case.coverage(ref)
    assert cov, "a case names at least one side"
    assert not E.covered(cov), {k: v for k, v in cov.items() if k in E.covered(cov)}
    assert case.branch and case.muts


@pytest.mark.parametrize("agent,name", ALL)
def test_the_f32_restatement_passes_every_bar_of_the_case(agent, name):
    """a correct f32 implementation can meet the bars: the committed restatement does, the derived element-wise ones included; and no
    bar is looser than the ceiling of the agent's GPU test file"""
    case, ref, f32out, checks = _case(agent, name)
    for c in checks:
        if c.against == "f64" and c.key in f32out:   # TorchSac keeps no q_pi / q_next / next_log_p
            assert c.ratio(f32out, ref) <= 1.0, (c.key, c.kind, c.err(f32out, ref), c.bar, c.how)
        if c.key.startswith("param") and c.kind == "elem":   # DQN: 0.3 lr but for a handful of entries whose terms cancel
            bars = np.asarray(c.bar[1])
            assert bars.min() == 0.3 * case.spec.lr and (bars > 0.3 * case.spec.lr).sum() <= 8 and bars.max() <= 2.0 * case.spec.lr, c.how
        if c.key.startswith("param") and c.kind == "abs":
            assert c.bar <= 0.3 * max(getattr(case.spec, k) for k in vars(case.spec) if k.startswith("lr")), (c.key, c.bar)
        if c.kind == "rel":
            top = 2e-3 if c.key.startswith(("grad", "w")) else 1e-4 if not c.key.startswith("param") else 1e-3 if agent == "dqn" else 1e-5
            assert c.bar <= top, (c.key, c.bar)
    for k in case.exact:   # exact means exact: the f32 restatement and float64 hold the same numbers
        assert k in f32out
        assert np.array_equal(np.asarray(f32out[k], np.float64), ref[k]), k


@pytest.mark.parametrize("agent,name,mut", TEETH)
def test_teeth_a_wrong_kernel_moves_some_quantity_by_ten_bars(agent, name, mut):
    case, ref, _, checks = _case(agent, name)
    bad = E.run_ref(case, mut=(mut,))
    worst = max(((c.ratio(bad, ref), c.key) for c in checks if c.against == "f64"), key=lambda t: t[0])
    assert worst[0] >= 10.0, (mut, worst)
