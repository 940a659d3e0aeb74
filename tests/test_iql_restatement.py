"""The IQL restatement (tests/iql_restatement.py) against a float64 numpy hand computation of one Iql::opt_ iteration
(border-candle-agent/src/iql/base.rs:157-188): the expectile loss, the TD target with is_truncated, logp in both action limits with the
log-Jacobian quirk, the softmax weights, and the order of the three steps.  CPU only."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import iql_restatement as R  # noqa: E402


def expectile_kat():
    # util.rs:262-266 on a known vector: tau = 0.7, u = [-2, -0.5, 0, 1, 3]
    u = np.array([-2.0, -0.5, 0.0, 1.0, 3.0])
    w = np.abs(0.7 - (u < 0))
    return u, float(np.mean(w * u * u))


def test_expectile_loss_known_answer():
    import torch
    u, want = expectile_kat()
    assert want == pytest.approx((0.3 * 4 + 0.3 * 0.25 + 0 + 0.7 * 1 + 0.7 * 9) / 5)
    t = torch.tensor(u, dtype=torch.float32)
    got = ((0.7 - (t < 0).float()).abs() * t ** 2).mean()
    assert float(got) == pytest.approx(want, rel=1e-6)


class Np64:
    """float64 numpy statement of the same update (forward + hand-derived backward), independent of autograd"""

    def __init__(self, spec, actor, critics, tgts, value):
        self.s = spec
        A = spec.act_dim
        self.actor = self._layers(actor[:-A], spec.obs_dim, spec.p_units, A)
        self.h2 = np.asarray(actor[-A:], np.float64)
        self.crit = [self._layers(c, spec.obs_dim + A, spec.q_units, 1) for c in critics]
        self.tgt = [self._layers(c, spec.obs_dim + A, spec.q_units, 1) for c in tgts]
        self.val = self._layers(value, spec.obs_dim, spec.v_units, 1)

    @staticmethod
    def _layers(flat, i, units, o):
        out, k = [], 0
        for (ro, ri), _ in R.mlp_shapes(i, units, o):
            W = np.asarray(flat[k:k + ro * ri], np.float64).reshape(ro, ri); k += ro * ri
            b = np.asarray(flat[k:k + ro], np.float64); k += ro
            out.append([W, b])
        return out

    @staticmethod
    def fwd(layers, x):
        hs = [x]
        for k, (W, b) in enumerate(layers):
            x = x @ W.T + b
            if k < len(layers) - 1:
                x = np.maximum(x, 0)
            hs.append(x)
        return x, hs

    @staticmethod
    def bwd(layers, hs, dy):
        grads = []
        for k in range(len(layers) - 1, -1, -1):
            W, _ = layers[k]
            grads.append([dy.T @ hs[k], dy.sum(0)])
            dy = (dy @ W) * (hs[k] > 0) if k > 0 else None
        return grads[::-1]

    @staticmethod
    def adam(layers_or_list, grads, state, lr, t):
        b1, b2, eps = 0.9, 0.999, 1e-8
        for li, (pl, gl) in enumerate(zip(layers_or_list, grads)):
            for j in range(len(pl)):
                key = (li, j)
                m, v = state.get(key, (0.0, 0.0))
                m = b1 * m + (1 - b1) * gl[j]; v = b2 * v + (1 - b2) * gl[j] ** 2
                state[key] = (m, v)
                pl[j] = pl[j] - lr / (1 - b1 ** t) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)

    def logp(self, obs, act):
        s = self.s
        mean, hs = self.fwd(self.actor, obs)
        ls = np.clip(self.h2, s.min_log_std, s.max_log_std)
        var = np.exp(ls) ** 2
        x = act if s.action_limit == "Clamp" else np.arctanh(np.clip(act / s.action_scale, -0.999999, 0.999999))
        lp = (-0.5 * math.log(2 * math.pi) - 0.5 * np.log(var) - (x - mean) ** 2 / (2 * var)).sum(1)
        if s.action_limit == "Tanh":   # 1 - a^2 at the clamp (a = 0.999999) is 2e-6: the value the reference's f32 arithmetic gives it
            a = np.clip(act.astype(np.float32), np.float32(-0.999999), np.float32(0.999999))
            lp = lp - np.log((np.float32(1) - a * a).astype(np.float64)).sum(1)
        return lp, mean, hs, x, var

    def update(self, obs, act, nxt, rew, term, trunc):
        s = self.s
        obs, act, nxt, rew = (np.asarray(z, np.float64) for z in (obs, act, nxt, rew))
        Bn, x = len(rew), np.concatenate([obs, act], 1)
        qmin = lambda nets: np.min([self.fwd(n, x)[0][:, 0] for n in nets], 0)
        # value
        q = qmin(self.tgt)
        v, hv = self.fwd(self.val, obs)
        u = q - v[:, 0]
        wt = np.abs(s.tau_iql - (u < 0))
        loss_value = np.mean(wt * u * u)
        gv = self.bwd(self.val, hv, (-2 * wt * u / Bn)[:, None])
        self.adam(self.val, gv, {}, s.lr_value, 1)
        # critic
        gnd = s.gamma * (1 - (np.asarray(term) | np.asarray(trunc)))
        tgt = rew + gnd * self.fwd(self.val, nxt)[0][:, 0]
        loss_critic = 0.0
        for c in self.crit:
            qc, hc = self.fwd(c, x)
            d = qc[:, 0] - tgt
            loss_critic += np.mean(d * d) / len(self.crit)
            self.adam(c, self.bwd(c, hc, (2 * d / (Bn * len(self.crit)))[:, None]), {}, s.lr_critic, 1)
        for c, t in zip(self.crit, self.tgt):
            for lc, lt in zip(c, t):
                for j in range(2):
                    lt[j] = s.critic_tau * lc[j] + (1 - s.critic_tau) * lt[j]
        # actor
        adv = qmin(self.tgt) - self.fwd(self.val, obs)[0][:, 0]
        z = s.inv_lambda * adv
        w = np.exp(z - z.max()) / np.exp(z - z.max()).sum() if s.adv_softmax else np.clip(np.exp(z), 0, s.exp_adv_max)
        lp, mean, hs, xa, var = self.logp(obs, act)
        loss_actor = np.mean(-lp * w)
        gmean = -(w / Bn)[:, None] * (xa - mean) / var
        gh2 = (-(w / Bn)[:, None] * ((xa - mean) ** 2 / var - 1)).sum(0)
        self.adam(self.actor, self.bwd(self.actor, hs, gmean), {}, s.lr_actor, 1)
        return dict(loss_value=loss_value, loss_critic=loss_critic, loss_actor=loss_actor, tgt=tgt, w=w, logp=lp, u=u, gh2=gh2)


@pytest.mark.parametrize("extra", [{}, {"action_limit": "Tanh", "action_scale": 2.0}, {"adv_softmax": True, "inv_lambda": 3.0}])
def test_one_update_matches_the_float64_hand_computation(extra):
    spec = R.IqlSpec(7, 3, (16, 12), (16,), (12, 16), **extra)
    params = spec.init_params(0)
    batch = R.make_batch(spec, 33, 5, p_done=0.3)
    ref = R.IqlRestatement(spec, *params)
    got = ref.update(*batch)
    want = Np64(spec, *params).update(*batch)
    for k in ("loss_value", "loss_critic", "loss_actor"):
        assert got[k] == pytest.approx(want[k], rel=2e-5, abs=1e-7), k
    pr = ref.probes
    for k in ("tgt", "w", "logp", "u"):
        np.testing.assert_allclose(pr[k], want[k], rtol=1e-4, atol=1e-5 * max(1.0, np.abs(want[k]).max()), err_msg=k)
    np.testing.assert_allclose(pr["actor_grad"][-3:], want["gh2"], rtol=1e-4, atol=1e-6)


def test_logp_tanh_jacobian_uses_the_action_not_action_over_scale():
    import torch
    spec = R.IqlSpec(4, 2, (8,), (8,), (8,), action_limit="Tanh", action_scale=3.0)
    params = spec.init_params(1)
    ref = R.IqlRestatement(spec, *params)
    obs = np.zeros((1, 4), np.float32)
    act = np.array([[0.9, -2.5]], np.float32)   # |a| > 1 for the second column: the clamp to 0.999999 shows in the Jacobian term
    lp = float(ref.logp(torch.tensor(obs), torch.tensor(act)).detach())
    want, mean, _, _, _ = Np64(spec, *params).logp(obs.astype(np.float64), act.astype(np.float64))
    assert lp == pytest.approx(float(want[0]), rel=1e-5)
    jac = -np.log(1 - np.clip(act.astype(np.float64), -0.999999, 0.999999) ** 2).sum()
    jac_scaled = -np.log(1 - (act / 3.0) ** 2).sum()
    assert abs(jac - jac_scaled) > 1.0   # the two readings differ: the test tells them apart


def test_update_order_value_then_critic_then_actor():
    """tgt uses the UPDATED value network; the actor's advantage uses the targets after the soft update."""
    spec = R.IqlSpec(5, 2, (8,), (8,), (8,), lr_value=0.05, critic_tau=0.5, lr_critic=0.05)
    params = spec.init_params(3)
    batch = R.make_batch(spec, 16, 9, p_done=0.0)
    ref = R.IqlRestatement(spec, *params)
    ref.update(*batch)
    pr = ref.probes
    old = Np64(spec, *params)
    v_old_next = old.fwd(old.val, batch[2].astype(np.float64))[0][:, 0]
    assert np.abs(pr["v_next"] - v_old_next).max() > 1e-4                   # not the value network of before the step
    assert np.abs(pr["q_tgt_min_actor"] - pr["q_tgt_min_value"]).max() > 1e-4  # the targets moved between steps 1 and 3
