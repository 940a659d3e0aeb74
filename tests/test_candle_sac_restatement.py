"""tests/candle_sac_restatement.py checked against itself, on the CPU:
  - the committed goldens are what the float32 restatement gives today (the generator is reproducible);
  - a float64 run of the same restatement on the same inputs: the float32-versus-float64 difference of gradients, logp, tgt and the
    other compared quantities is printed per case and step (pytest -s) - the GPU bars of tests/test_gpu_candle_sac.py refer to
    these numbers - and bounded loosely, so that a restatement that is ill-conditioned on its own inputs shows here first;
  - mutation checks: each deliberate departure from the reference moves a compared quantity by at least 10 bars on at least one
    committed case, so the GPU test would see it;
  - the pieces the reference pins: Mlp2's double exponential, ReLU after the last trunk layer, the tie rule, EntCoef's AdamW step."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import candle_sac_restatement as R  # noqa: E402
import make_golden_candle_sac as MG  # noqa: E402

# the bars of tests/test_gpu_candle_sac.py (tests/test_gpu_awac.py's): max-relative, but the parameters (x lr, absolute)
BARS = dict(actor_grad=2e-3, critic_grad=2e-3, a=1e-4, logp=1e-4, q_min=1e-4, dq_da=1e-4, next_a=1e-4, next_logp=1e-4, tgt=1e-4, q_pred=1e-4)

# A committed case beyond the goldens' precondition: draws six times N(0,1) with std >= 1 drive tanh to +-1 in float32 on most rows,
# where only the clamp inside atanh keeps logp finite.
SATURATED = (R.CandleSacSpec(5, 2, (16, 16), (16,), actor_kind="Mlp2", action_limit="Tanh", action_scale=2.0, ent_coef=("Fix", 0.2)), 8, 9)


def _run(name, mutate=(), dtype=torch.float32):
    """the per-step probes (+ parameters) of a restatement on the committed case `name`"""
    spec, bsz, steps, seed = MG.case(name)
    ref = R.CandleSacRestatement(spec, *MG.initial(name), dtype=dtype, mutate=mutate)
    out = []
    for s in range(steps):
        batch, z_pi, z_next = MG.inputs(name, s)
        rec = ref.update(*batch, z_pi, z_next)
        pr = dict(ref.probes)
        pr.update(rec=rec, actor=ref.params("actor"), critic_grad=np.concatenate(pr["critic_grads"]),
                  critic=np.concatenate([ref.params(f"critic_{i}") for i in range(spec.n_critics)]))
        out.append(pr)
    return out, ref


@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_goldens_are_reproducible_and_the_float64_figures(golden_dir, name):
    spec, bsz, steps, seed = MG.case(name)
    g = np.load(os.path.join(golden_dir, f"candle_sac_{name}.npz"))
    run, ref = _run(name)
    ref64 = R.CandleSacRestatement(spec, *MG.initial(name), dtype=torch.float64)
    ref32 = R.CandleSacRestatement(spec, *MG.initial(name))
    for s in range(steps):
        for k in MG.PROBE_KEYS + ("actor_grad", "actor"):
            assert R.rel(run[s][k], g[f"s{s}_{k}"]) < 1e-5, (name, s, k)      # (another BLAS may round the sums differently)
        batch, z_pi, z_next = MG.inputs(name, s)
        ref32.update(*batch, z_pi, z_next); ref64.update(*batch, z_pi, z_next)
        fig = R.f32_f64_figures(ref32, ref64)
        print(f"candle_sac {name} step {s} f32-vs-f64: " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
        for k in ("actor_grad", "critic_grad"):
            assert fig[k] < 2e-3, (name, s, k, fig[k])          # inside the GPU bar: the bar is the AWAC one
        for k in ("a", "next_a", "q_min", "q_pred", "dq_da"):
            assert fig[k] < 1e-5, (name, s, k, fig[k])
        # logp / tgt: the Tanh limit's log-Jacobian clamps the action ITSELF at 0.999999, whose float32 neighbour is 0.99999899:
        # ln(1 - a^2) moves by 1.3e-2 per clamped element (action_scale 2: |a| > 1 on many rows).  Anything beyond that is a defect.
        lim = 5e-3 if spec.action_limit == "Tanh" and spec.action_scale > 1.0 else 1e-5
        for k in ("logp", "next_logp", "tgt"):
            assert fig[k] < lim, (name, s, k, fig[k])


def _moves(name, mutation, key):
    """by how many bars does `mutation` move `key` on the committed case, at its worst step"""
    base, _ = _run(name)
    mut, _ = _run(name, (mutation,))
    g = np.load(os.path.join(MG.HERE, f"candle_sac_{name}.npz"))
    worst = 0.0
    for s, (b, m) in enumerate(zip(base, mut)):
        bar = max(BARS[key], 4.0 * float(g[f"s{s}_fig_{key}"]))
        worst = max(worst, R.rel(m[key], b[key]) / bar)
    return worst


@pytest.mark.parametrize("mutation,name,key", [
    ("jacobian_on_a_over_scale", "mlp2_tanh_auto_smooth_l1", "logp"),        # action_scale 2
    ("single_exp", "mlp2_clamp_fix_mse_adamw", "a"),
    ("alpha_before_update", "mlp3_tanh_auto_three_critics", "tgt"),          # Auto, lr 1e-2
    ("target_with_old_actor", "mlp2_clamp_fix_mse_adamw", "next_a"),         # lr_actor 1e-3
    ("sum_over_critics", "mlp3_tanh_auto_three_critics", "critic_grad"),
    ("count_is_truncated", "mlp2_clamp_fix_mse_adamw", "tgt"),
    ("argmin", "mlp2_clamp_identical_critics", "dq_da"),
])
def test_each_mutation_moves_a_compared_quantity_by_ten_bars(mutation, name, key):
    n = _moves(name, mutation, key)
    print(f"candle_sac mutation {mutation} on {name}: {key} moves by {n:.1f} bars")
    assert n >= 10.0, (mutation, name, key, n)


def test_dropping_the_atanh_clamp_shows_on_the_saturated_case():
    """the goldens stay off saturation by their precondition, where the clamp is idle: the committed case for this mutation is SATURATED"""
    spec, bsz, seed = SATURATED
    params = spec.init_params(seed)
    batch = R.make_batch(spec, bsz, seed)
    z = spec.draws(bsz, seed + 1, 6.0)
    ref = R.CandleSacRestatement(spec, *params)
    mut = R.CandleSacRestatement(spec, *params, mutate=("atanh_clamp_dropped",))
    ref.update(*batch, *z)
    mut.update(*batch, *z)
    assert (np.abs(ref.probes["a"]) == spec.action_scale).any()                 # tanh reached +-1 in float32
    assert np.isfinite(ref.probes["logp"]).all() and np.isfinite(ref.probes["actor_grad"]).all() and np.isfinite(ref.probes["tgt"]).all()
    assert not np.isfinite(mut.probes["logp"]).all()                             # atanh(1) without the clamp: far beyond 10 bars


# ---------------------------------------------------------------------------------------------------------- the pieces
def test_mlp2_keeps_the_double_exponential_and_the_relu_after_the_last_trunk_layer():
    spec = R.CandleSacSpec(4, 2, (8, 6), (8,), actor_kind="Mlp2", action_min=-100.0, action_max=100.0)
    actor, critics, tgts = spec.init_params(3)
    ref = R.CandleSacRestatement(spec, actor, critics, tgts)
    obs = torch.as_tensor(np.random.default_rng(0).standard_normal((7, 4)).astype(np.float32))
    w0, b0, w1, b1 = [p.detach() for p in ref.trunk.params]
    wm, bm, ws, bs = [p.detach() for p in ref.heads]
    h = torch.relu(torch.relu(obs @ w0.T + b0) @ w1.T + b1)                      # mlp.rs:14-24 with Activation::ReLU
    mean, l = ref.dist(obs)
    assert torch.equal(mean.detach(), h @ wm.T + bm) and torch.equal(l.detach(), (h @ ws.T + bs).exp())   # mlp2.rs:40-41
    z = np.ones((7, 2), np.float32)
    std = (ref.sample(obs.numpy(), z) - ref.sample(obs.numpy())) / z
    want = l.detach().clamp(-20.0, 2.0).exp().numpy()                            # util/actor.rs:228: exp(clamp(exp(s)))
    assert np.abs(std - want).max() < 1e-5 and (want >= 1.0).all() and (want <= math.e ** 2 + 1e-5).all()


def test_the_minimum_passes_its_gradient_to_every_equal_critic():
    qs = torch.tensor([[1.0, 2.0, 3.0], [1.0, 5.0, 0.5], [4.0, 2.0, 0.5]], requires_grad=True)
    q = R.MinTie.apply(qs)
    assert q.tolist() == [1.0, 2.0, 0.5]
    q.sum().backward()
    assert qs.grad.tolist() == [[1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]   # ties: both; torch.min(0) would pick one


def test_ent_coef_auto_is_one_adamw_step_on_minus_mean_logp_plus_target_entropy():
    spec = R.CandleSacSpec(4, 2, (8, 8), (8,), actor_kind="Mlp3", ent_coef=("Auto", -2.0, 1e-2))
    params = spec.init_params(1)
    ref = R.CandleSacRestatement(spec, *params)
    batch = R.make_batch(spec, 6, 2)
    rec = ref.update(*batch, *spec.draws(6, 3))
    g = -(ref.probes["logp"].astype(np.float64) + (-2.0)).mean()
    assert abs(float(ref.probes["log_alpha_grad"][0]) - g) < 1e-6 * max(1.0, abs(g))
    # first AdamW step from log_alpha = 0: the decay leaves 0, the update is -lr sign(g) (m / sqrt(v) = +-1 after bias correction)
    want = -1e-2 * np.sign(g)
    assert abs(float(ref.params("log_alpha")[0]) - want) < 1e-6
    assert abs(rec["ent_coef"] - math.exp(want)) < 1e-6
    fix = R.CandleSacRestatement(R.CandleSacSpec(4, 2, (8, 8), (8,), ent_coef=("Fix", 0.2)), *R.CandleSacSpec(4, 2, (8, 8), (8,)).init_params(1))
    assert fix.params("log_alpha")[0] == np.float32(math.log(0.2)) and fix.opt_alpha is None
