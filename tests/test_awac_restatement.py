"""The AWAC restatement (tests/awac_restatement.py) against a float64 numpy hand computation of one Awac::opt_ iteration
(border-candle-agent/src/awac/base.rs:170-215): the advantage from the ONLINE critics, the weights (clamped exp and softmax), logp in
both action limits, the SUM of the critic losses, the TD target with is_truncated, the order of the two steps and the record's
sum-versus-mean quirk.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import awac_restatement as R  # noqa: E402
from iql_restatement import mlp_shapes  # noqa: E402


def _layers(flat, i, units, o):
    out, k = [], 0
    for (ro, ri), _ in mlp_shapes(i, units, o):
        W = np.asarray(flat[k:k + ro * ri], np.float64).reshape(ro, ri); k += ro * ri
        b = np.asarray(flat[k:k + ro], np.float64); k += ro
        out.append([W, b])
    return out


def fwd(layers, x, relu_out=False):
    hs = [x]
    for k, (W, b) in enumerate(layers):
        x = x @ W.T + b
        if k < len(layers) - 1 or relu_out:
            x = np.maximum(x, 0)
        hs.append(x)
    return x, hs


def bwd(layers, hs, dy):
    grads = []
    for k in range(len(layers) - 1, -1, -1):
        W, _ = layers[k]
        grads.append([dy.T @ hs[k], dy.sum(0)])
        dy = (dy @ W) * (hs[k] > 0) if k > 0 else None
    return grads[::-1]


def adam(params, grads, lr, t=1):
    b1, b2, eps = 0.9, 0.999, 1e-8
    for pl, gl in zip(params, grads):
        for j in range(len(pl)):
            m = (1 - b1) * gl[j]; v = (1 - b2) * gl[j] ** 2
            pl[j] = pl[j] - lr / (1 - b1 ** t) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)


class Np64:
    """float64 numpy statement of one AWAC update (forward + hand-derived backward), independent of autograd"""

    def __init__(self, spec, actor, critics, tgts):
        self.s = spec
        A = spec.act_dim
        self.actor = _layers(actor[:-A], spec.obs_dim, spec.p_units, A)
        self.h2 = [np.asarray(actor[-A:], np.float64)]
        self.crit = [_layers(c, spec.obs_dim + A, spec.q_units, 1) for c in critics]
        self.tgt = [_layers(c, spec.obs_dim + A, spec.q_units, 1) for c in tgts]

    def std(self):
        return np.exp(np.clip(self.h2[0], self.s.min_log_std, self.s.max_log_std))

    def sample(self, obs, z):
        s = self.s
        a = fwd(self.actor, obs)[0] + (0 if z is None else self.std() * np.asarray(z, np.float64))
        return np.clip(a, s.action_min, s.action_max) if s.action_limit == "Clamp" else s.action_scale * np.tanh(a)

    def logp(self, obs, act):
        s = self.s
        mean, hs = fwd(self.actor, obs)
        var = self.std() ** 2
        x = act if s.action_limit == "Clamp" else np.arctanh(np.clip(act / s.action_scale, -0.999999, 0.999999))
        lp = (-0.5 * math.log(2 * math.pi) - 0.5 * np.log(var) - (x - mean) ** 2 / (2 * var)).sum(1)
        if s.action_limit == "Tanh":
            a = np.clip(act.astype(np.float32), np.float32(-0.999999), np.float32(0.999999))
            lp = lp - np.log((np.float32(1) - a * a).astype(np.float64)).sum(1)
        return lp, mean, hs, x, var

    def update(self, obs, act, nxt, rew, term, trunc, z_pi, z_next):
        s = self.s
        obs, act, nxt, rew = (np.asarray(z, np.float64) for z in (obs, act, nxt, rew))
        Bn = len(rew)
        qmin = lambda nets, o, a: np.min([fwd(n, np.concatenate([o, a], 1), s.q_relu_out)[0][:, 0] for n in nets], 0)
        # update_actor
        act_ = self.sample(obs, z_pi)
        q, v = qmin(self.crit, obs, act), qmin(self.crit, obs, act_)
        adv = q - v
        z = s.inv_lambda * adv
        w = np.exp(z - z.max()) / np.exp(z - z.max()).sum() if s.adv_softmax else np.clip(np.exp(z), 0, s.exp_adv_max)
        lp, mean, hs, xa, var = self.logp(obs, act)
        loss_actor = np.mean(-lp * w)
        gmean = -(w / Bn)[:, None] * (xa - mean) / var
        h2 = self.h2[0]
        gh2 = (-(w / Bn)[:, None] * ((xa - mean) ** 2 / var - 1)).sum(0) * ((h2 >= s.min_log_std) & (h2 <= s.max_log_std))
        adam(self.actor + [self.h2], bwd(self.actor, hs, gmean) + [[gh2]], s.lr_actor)
        # update_critic with the updated actor
        next_act = self.sample(nxt, z_next)
        next_q = qmin(self.tgt, nxt, next_act)
        gnd = s.gamma * (1 - (np.asarray(term) | np.asarray(trunc)))
        tgt = rew + gnd * next_q
        x = np.concatenate([obs, act], 1)
        loss_critic = 0.0
        for c in self.crit:
            qc, hc = fwd(c, x, s.q_relu_out)
            d = qc[:, 0] - tgt
            if s.critic_loss == "Mse":
                loss_critic += np.mean(d * d); g = 2 * d / Bn
            else:
                ad = np.abs(d); loss_critic += np.mean(np.where(ad < 1, 0.5 * d * d, ad - 0.5)); g = np.where(ad < 1, d, np.sign(d)) / Bn
            if s.q_relu_out:
                g = g * (qc[:, 0] > 0)
            adam(c, bwd(c, hc, g[:, None]), s.lr_critic)
        for c, t in zip(self.crit, self.tgt):
            for lc, lt in zip(c, t):
                for j in range(2):
                    lt[j] = s.critic_tau * lc[j] + (1 - s.critic_tau) * lt[j]
        return dict(loss_actor=loss_actor, loss_critic=loss_critic, adv=adv, w=w, logp=lp, tgt=tgt, next_act=next_act, next_q=next_q,
                    gh2=gh2, q_tgt_abs_mean=np.abs(tgt).mean(), adv_mean=adv.mean(), adv_abs_mean=np.abs(adv).mean(), logp_mean=lp.mean(),
                    reward_mean=rew.mean(), next_q_mean=next_q.mean())


CASES = [{}, {"action_limit": "Tanh", "action_scale": 2.0, "critic_loss": "SmoothL1"}, {"adv_softmax": True, "inv_lambda": 3.0, "n_critics": 3}]


@pytest.mark.parametrize("extra", CASES)
def test_one_update_matches_the_float64_hand_computation(extra):
    spec = R.AwacSpec(7, 3, (16, 12), (12, 16), **extra)
    params = spec.init_params(0)
    batch = R.make_batch(spec, 33, 5, p_done=0.3)
    z = spec.draws(33, 6)
    ref = R.AwacRestatement(spec, *params)
    got = ref.update(*batch, *z)
    want = Np64(spec, *params).update(*batch, *z)
    for k in R.RECORD_KEYS:
        assert got[k] == pytest.approx(want[k], rel=2e-5, abs=1e-6), k
    pr = ref.probes
    for k in ("adv", "w", "logp", "tgt", "next_act", "next_q"):
        np.testing.assert_allclose(pr[k], want[k], rtol=1e-4, atol=1e-5 * max(1.0, np.abs(want[k]).max()), err_msg=k)
    np.testing.assert_allclose(pr["actor_grad"][-3:], want["gh2"], rtol=1e-4, atol=1e-6)


def test_the_advantage_uses_the_online_critics_not_the_targets():
    spec = R.AwacSpec(5, 2, (8,), (8,))
    actor, critics, _ = spec.init_params(2)
    tgts = [c * 0.5 for c in critics]   # targets that differ from the critics
    batch = R.make_batch(spec, 16, 3)
    z = spec.draws(16, 4)
    ref = R.AwacRestatement(spec, actor, critics, tgts)
    ref.update(*batch, *z)
    old = Np64(spec, actor, critics, tgts)
    q_online = np.min([fwd(c, np.concatenate([batch[0], batch[1]], 1).astype(np.float64))[0][:, 0] for c in old.crit], 0)
    np.testing.assert_allclose(ref.probes["q_data_min"], q_online, rtol=1e-5, atol=1e-6)


def test_update_order_actor_then_critic():
    """next_act of the critic step is sampled from the actor AFTER its step; the critic predictions are those of before the step."""
    spec = R.AwacSpec(5, 2, (8,), (8,), lr_actor=0.05, lr_critic=0.05)
    params = spec.init_params(3)
    batch = R.make_batch(spec, 16, 9, p_done=0.0)
    z_pi, z_next = spec.draws(16, 1)
    ref = R.AwacRestatement(spec, *params)
    before = R.AwacRestatement(spec, *params)
    ref.update(*batch, z_pi, z_next)
    pr = ref.probes
    with_old = before.sample(batch[2], z_next).numpy()
    assert np.abs(pr["next_act"] - with_old).max() > 1e-3                # not the actor of before the step
    after = R.AwacRestatement(spec, ref.params("actor"), params[1], params[2])
    np.testing.assert_array_equal(pr["next_act"], after.sample(batch[2], z_next).numpy())   # the updated actor
    x = np.concatenate([batch[0], batch[1]], 1).astype(np.float32)
    import torch
    q_old = before.critics[0].forward(torch.tensor(x)).squeeze(-1).detach().numpy()
    np.testing.assert_array_equal(pr["q_pred"][0], q_old)                # the critics had not moved when the actor step ran


def test_eval_mode_uses_the_means():
    spec = R.AwacSpec(6, 3, (8,), (8,), action_min=-0.2, action_max=0.3)
    params = spec.init_params(5)
    batch = R.make_batch(spec, 12, 2)
    ref = R.AwacRestatement(spec, *params)
    probe = R.AwacRestatement(spec, *params)
    ref.update(*batch)
    np.testing.assert_array_equal(ref.probes["act_"], probe.sample(batch[0]).numpy())


def test_critic_loss_is_the_sum_over_critics():
    spec = R.AwacSpec(5, 2, (8,), (8,), n_critics=3)
    params = spec.init_params(4)
    batch = R.make_batch(spec, 20, 1)
    ref = R.AwacRestatement(spec, *params)
    rec = ref.update(*batch, *spec.draws(20, 2))
    pr = ref.probes
    per = [float(np.mean((pr["q_pred"][i].astype(np.float64) - pr["tgt"]) ** 2)) for i in range(3)]
    assert rec["loss_critic"] == pytest.approx(sum(per), rel=1e-5)
    assert rec["loss_critic"] > 2.5 * min(per)   # not their mean


def test_record_averages_five_keys_and_sums_three_over_three_updates():
    spec = R.AwacSpec(6, 2, (8,), (8,))
    params = spec.init_params(7)
    ref = R.AwacRestatement(spec, *params)
    recs = [ref.update(*R.make_batch(spec, 10, 20 + k), *spec.draws(10, 30 + k)) for k in range(3)]
    out = ref.opt_record(recs)
    for i, k in enumerate(R.RECORD_KEYS):
        total = sum(r[k] for r in recs)
        assert out[k] == pytest.approx(total / 3 if i < 5 else total, rel=1e-6), k
    assert list(out) == list(R.RECORD_KEYS)
    assert abs(out["reward_mean"] - sum(r["reward_mean"] for r in recs) / 3) > 1e-3   # the two readings differ here


def test_is_truncated_counts_in_gamma_not_done():
    spec = R.AwacSpec(4, 2, (8,), (8,))
    params = spec.init_params(1)
    obs, act, nxt, rew, _, _ = R.make_batch(spec, 8, 4)
    ref = R.AwacRestatement(spec, *params)
    ref.update(obs, act, nxt, rew, np.zeros(8, np.int8), np.ones(8, np.int8), *spec.draws(8, 1))
    np.testing.assert_array_equal(ref.probes["tgt"], rew)
