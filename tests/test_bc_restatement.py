"""The BC restatement (tests/bc_restatement.py) against a float64 numpy hand computation of one Bc::opt_
(border-candle-agent/src/bc/base.rs:167-198): every output activation with its hand-derived derivative, both optimizers, the mean
over all B x A elements, and the Discrete refusal.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import bc_restatement as R  # noqa: E402
from iql_restatement import mlp_shapes  # noqa: E402

ADAMW = dict(beta1=0.85, beta2=0.99, eps=1e-7, wd=0.02)


def _layers(flat, i, units, o):
    out, k = [], 0
    for (ro, ri), _ in mlp_shapes(i, units, o):
        W = np.asarray(flat[k:k + ro * ri], np.float64).reshape(ro, ri); k += ro * ri
        b = np.asarray(flat[k:k + ro], np.float64); k += ro
        out.append([W, b])
    return out


def _act(kind, z):
    """y and dy/dz"""
    if kind == "None":
        return z, np.ones_like(z)
    if kind == "ReLU":
        return np.maximum(z, 0), (z > 0).astype(np.float64)
    if kind == "Tanh":
        y = np.tanh(z)
        return y, 1 - y * y
    y = 1 / (1 + np.exp(-z))
    return y, y * (1 - y)


def hand_update(spec, flat, obs, act):
    """float64: forward, the hand-derived backward, one Adam / AdamW step at t = 1 -> (loss, pred, dz, grads flat, params flat)"""
    layers = _layers(flat, spec.obs_dim, spec.units, spec.act_dim)
    hs, x = [np.asarray(obs, np.float64)], np.asarray(obs, np.float64)
    for k, (W, b) in enumerate(layers):
        x = x @ W.T + b
        if k < len(layers) - 1:
            x = np.maximum(x, 0)
            hs.append(x)
    y, gp = _act(spec.activation_out, x)
    d = y - np.asarray(act, np.float64)
    n = d.size                                   # B x A
    loss = (d * d).sum() / n
    dz = 2 * d / n * gp
    grads, dy = [], dz
    for k in range(len(layers) - 1, -1, -1):
        grads.append([dy.T @ hs[k], dy.sum(0)])
        if k > 0:
            dy = (dy @ layers[k][0]) * (hs[k] > 0)
    grads = grads[::-1]
    if spec.adamw is None:
        b1, b2, eps, wd = 0.9, 0.999, 1e-8, 0.0
    else:
        b1, b2, eps, wd = (spec.adamw[k] for k in ("beta1", "beta2", "eps", "wd"))
    new = []
    for pl, gl in zip(layers, grads):
        for p, g in zip(pl, gl):
            m, v = (1 - b1) * g, (1 - b2) * g * g
            p = p * (1 - spec.lr * wd)
            new.append(p - spec.lr / (1 - b1) * m / (np.sqrt(v) / math.sqrt(1 - b2) + eps))
    flat_g = np.concatenate([g.reshape(-1) for gl in grads for g in gl])
    return loss, y, dz, flat_g, np.concatenate([p.reshape(-1) for p in new])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("adamw", [None, ADAMW])
@pytest.mark.parametrize("kind", ["None", "ReLU", "Tanh", "Sigmoid"])
def test_one_update_against_the_float64_hand_computation(kind, adamw):
    spec = R.BcSpec(7, 3, (12, 10), kind, lr=1e-2, adamw=adamw)
    flat = spec.init_params(3)
    obs, act = R.make_batch(spec, 9, 5)
    ref = R.BcRestatement(spec, flat)
    rec = ref.update(obs, act)
    loss, y, dz, g, p = hand_update(spec, flat, obs, act)
    assert abs(rec["loss"] - loss) <= 1e-5 * abs(loss)
    assert rel(ref.probes["pred"], y) < 1e-5 and rel(ref.probes["dz"], dz) < 1e-4
    assert rel(ref.probes["grad"], g) < 1e-4
    # Adam's first step moves every parameter by about lr whatever the gradient's size: compare the steps, not the parameters
    assert np.abs(ref.params() - p).max() < 1e-3 * spec.lr


def test_the_loss_is_the_mean_over_all_elements_not_over_rows():
    spec = R.BcSpec(5, 4, (8,), "None")
    flat = spec.init_params(1)
    obs, act = R.make_batch(spec, 6, 2)
    ref = R.BcRestatement(spec, flat)
    pred = ref.forward(obs).detach().numpy().astype(np.float64)
    sq = (pred - act) ** 2
    rec = ref.update(obs, act)
    assert abs(rec["loss"] - sq.sum() / (6 * 4)) < 1e-6 * sq.sum()
    assert abs(rec["loss"] - sq.sum() / 6) > 0.5 * rec["loss"]       # the per-row mean would be A times larger


def test_a_discrete_spec_refuses_to_update_and_samples_the_argmax():
    spec = R.BcSpec(5, 4, (8,), "None", action_type="Discrete")
    ref = R.BcRestatement(spec, spec.init_params(1))
    obs, act = R.make_batch(spec, 6, 2)
    with pytest.raises(RuntimeError, match="Discrete"):
        ref.update(obs, act)
    idx = ref.sample(obs)
    assert idx.dtype == np.int64 and idx.shape == (6,)
    assert (idx == ref.forward(obs).detach().numpy().argmax(-1)).all()


def test_goldens_are_what_the_restatement_computes(golden_dir):
    sys.path.insert(0, golden_dir)
    import make_golden_bc as MG
    for name in MG.CASES:
        spec, bsz, steps, seed = MG.case(name)
        g = np.load(os.path.join(golden_dir, f"bc_{name}.npz"))
        assert os.path.getsize(os.path.join(golden_dir, f"bc_{name}.npz")) <= 259 * 1024
        ref = R.BcRestatement(spec, g["policy0"])
        for s in range(steps):
            rec = ref.update(g[f"s{s}_obs"], g[f"s{s}_act"])
            assert abs(rec["loss"] - float(g[f"s{s}_loss"])) <= 1e-5 * abs(rec["loss"]), (name, s)
            assert np.abs(ref.params() - g[f"s{s}_policy"]).max() < 0.05 * spec.lr, (name, s)
