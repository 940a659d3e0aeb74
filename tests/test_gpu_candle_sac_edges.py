"""The candle SAC kernels' clamp, kink, tie and saturation branches on the GPU (csrc/candle_sac.hip), with dial networks in the style
of DESIGN section 12 (tests/edge_inputs.py: dial_mlp, const_mlp): the actor's mean is exactly one observation column, Mlp2's s
another one, a critic's value exactly gain x the action, so every branch is reached by writing the input that reaches it.

References are float64: tests/candle_sac_restatement.py run in float64 with the reference's float32 clamp constant
(edge_inputs.CLAMP1).  With the Tanh limit the float64 run takes the DEVICE's tanh values (R.TanhGiven; they are the probe `a`,
action_scale = 1) and the test checks those against float64 tanh separately, within 4 float32 ulp: near saturation one ulp of
tanh moves 1 - tanh^2 by percents, and that conditioning is not the kernel's.
Bars: those of tests/test_gpu_candle_sac.py - probes 1e-4, gradients 2e-3 max-relative - or 4 x the distance of the float32
restatement from the float64 one on the same case where that is larger (R.f32_f64_figures), written beside each assertion.
Where the reference's gradient is exactly 0 the device's must be == 0.
The rule for a clamp's gradient ON its bound (closed range, gradient 1: tests/edge_inputs.py header) is the restatement's, PyTorch's."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import candle_sac_restatement as R  # noqa: E402
from edge_inputs import CLAMP1, const_mlp, dial_mlp  # noqa: E402

O, N = 4, 8            # observation columns: 0 -> the mean, 1 -> Mlp2's s, 2 -> the critics' observation term; rows per batch
PU, QU = (8, 8), (8,)  # hidden widths: at least two units per dialled term


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def mlp2_reference_order(flat, H, A):
    """an Mlp of width 2 A at the end (rows: mean, then s) -> Mlp2's reference layout: trunk, mean.weight, mean.bias, std.weight, std.bias"""
    n = 2 * A * H + 2 * A
    t, w, b = flat[:-n], flat[-n:-2 * A].reshape(2 * A, H), flat[-2 * A:]
    return np.concatenate([t, w[:A].reshape(-1), b[:A], w[A:].reshape(-1), b[A:]]).astype(np.float32)


def dial_actor(kind, A=1, head2=None, s_bias=None, mean_gain=1.0):
    """mean_j = mean_gain x obs[:, 0]; Mlp3: head2 as given; Mlp2: s_j = obs[:, 1] (+ s_bias)"""
    units = (4 * A + 4, 4 * A + 4)
    if kind == "Mlp3":
        return np.concatenate([dial_mlp(O, units, A, [0] * A, mean_gain), np.asarray(head2, np.float32)]), units
    bias = None if s_bias is None else [0.0] * A + list(s_bias)
    flat = dial_mlp(O, units, 2 * A, [[(0, mean_gain)]] * A + [[(1, 1.0)]] * A, bias=bias)
    return mlp2_reference_order(flat, units[-1], A), units


def dial_critic(A, gain, obs_gain=0.0):
    """Q = gain x a_0 (+ obs_gain x obs[:, 2]): dQ/da_0 = gain exactly"""
    terms = [(O, gain)] + ([(2, obs_gain)] if obs_gain else [])
    return dial_mlp(O + A, QU, 1, [terms])


def batch(mean_col, s_col=None, obs2=None, next_mean=None, term=None, seed=0):
    rng = np.random.default_rng(seed)
    n = len(mean_col)
    obs = np.zeros((n, O), np.float32); nxt = np.zeros((n, O), np.float32)
    obs[:, 0] = mean_col
    nxt[:, 0] = mean_col[::-1] if next_mean is None else next_mean
    if s_col is not None:
        obs[:, 1] = s_col; nxt[:, 1] = s_col[::-1]
    obs[:, 2] = rng.standard_normal(n) if obs2 is None else obs2
    nxt[:, 2] = rng.standard_normal(n)
    rew = rng.standard_normal(n).astype(np.float32)
    term = np.zeros(n, np.int8) if term is None else np.asarray(term, np.int8)
    return obs, None, nxt, rew, term, np.zeros(n, np.int8)


def run(B, spec, params, rows, z, A=1, train=True, given_tanh=False):
    """one update on the device and on the float64 / float32 restatements; returns (agent, ref64, ref32, figures)"""
    obs, _, nxt, rew, term, trunc = rows
    act = np.random.default_rng(5).uniform(-0.5, 0.5, (len(rew), A)).astype(np.float32)
    a = B.CandleSac.build(spec.to_config(B, len(rew), device=0, train=train))
    actor, critics, tgts = params
    a.set_params(actor, "actor")
    for i in range(spec.n_critics):
        a.set_params(critics[i], f"critic_{i}"); a.set_params(tgts[i], f"critic_tgt_{i}")
    zz = z if train else (None, None)
    a.update_on_batch(obs, act, nxt, rew, term, trunc, *zz)
    n = len(rew)
    given = None
    if given_tanh:
        assert spec.action_scale == 1.0
        given = [a.probe("a", n).astype(np.float64), a.probe("next_a", n).astype(np.float64)]
    r64 = R.CandleSacRestatement(spec, *params, dtype=torch.float64, clamp1=CLAMP1, tanh_given=given)
    r32 = R.CandleSacRestatement(spec, *params, tanh_given=given)
    for r in (r64, r32):
        r.update(obs, act, nxt, rew, term, trunc, *zz)
    return a, r64, r32, R.f32_f64_figures(r32, r64)


def bar(base, fig):
    return max(base, 4.0 * float(fig))


def compare(a, r64, fig, spec, n, tag, probes=("a", "logp", "q_min", "dq_da", "next_a", "next_logp", "tgt")):
    pr = r64.probes
    for k in probes:
        got = a.probe(k, n)
        assert np.isfinite(got).all(), (tag, k)
        print(tag, k, R.rel(got, pr[k]), "bar", bar(1e-4, fig[k]))
        assert R.rel(got, pr[k]) < bar(1e-4, fig[k]), (tag, k, R.rel(got, pr[k]), fig[k])           # probes 1e-4, or 4 x fig
    for name, want, key in [("actor", pr["actor_grad"], "actor_grad")] + [(f"critic_{i}", pr["critic_grads"][i], "critic_grad") for i in range(spec.n_critics)]:
        g = a.get_params(name, "grad")
        assert np.isfinite(g).all(), (tag, name)
        assert (g[want == 0.0] == 0.0).all(), (tag, name, "a gradient the reference has exactly 0")
        if np.abs(want).max() > 0:
            print(tag, name, R.rel(g, want), "bar", bar(2e-3, fig[key]))
            assert R.rel(g, want) < bar(2e-3, fig[key]), (tag, name, R.rel(g, want), fig[key])       # gradients 2e-3, or 4 x fig


def base_spec(kind, **kw):
    d = dict(actor_kind=kind, p_units=PU, q_units=QU, ent_coef=("Fix", 0.5))
    d.update(kw)
    return R.CandleSacSpec(O, d.pop("A", 1), **d)


# ---------------------------------------------------------------------------------------------------------- the Tanh limit
def _u_at_clamp1(B):
    """observation values u with tanhf(u) == CLAMP1 and tanhf(-u) == -CLAMP1 ON THE DEVICE, found by sampling: near atanh(CLAMP1) =
    7.25 one float32 step of tanh spans 0.03 of u, so a 1e-4 grid crosses every float32 value of tanh there many times"""
    spec = base_spec("Mlp3", action_limit="Tanh")
    actor, units = dial_actor("Mlp3", head2=[0.0])
    spec.p_units = units
    a = B.CandleSac.build(spec.to_config(B, 2, device=0, train=False))
    a.set_params(actor, "actor")
    u = np.linspace(7.0, 7.6, 6001).astype(np.float32)
    obs = np.zeros((2 * len(u), O), np.float32)
    obs[:len(u), 0], obs[len(u):, 0] = u, -u
    act = a.sample(obs).reshape(-1)
    a.close()
    hit = (act[:len(u)] == np.float32(CLAMP1)) & (act[len(u):] == -np.float32(CLAMP1))
    if not hit.any():
        pytest.fail("no observation reaches tanh == +-0.999999 exactly on this device")
    return float(u[np.flatnonzero(hit)[len(np.flatnonzero(hit)) // 2]])


@pytest.mark.parametrize("kind", ["Mlp3", "Mlp2"])
def test_tanh_limit_below_at_and_above_the_atanh_clamp(B, kind):
    """a / scale below (|u| = 6.5), exactly at (found on the device) and above (|u| = 7.5; 20: tanh == 1) +-0.999999, both signs.
    z = 0 on those rows keeps u = the dialled mean bit for bit; row 0 is an ordinary one with z != 0."""
    ua = _u_at_clamp1(B)
    spec = base_spec(kind, action_limit="Tanh", action_scale=1.0)
    actor, spec.p_units = dial_actor(kind, head2=[0.0])
    mean = np.array([0.3, 6.5, -6.5, ua, -ua, 7.5, -7.5, 20.0], np.float32)
    rows = batch(mean, s_col=np.full(N, -30.0, np.float32))      # Mlp2: l = exp(-30) ~ 0, inside [-20, 2]: sd = 1
    z = np.zeros((N, 1), np.float32); z[0] = 0.4
    crit = [dial_critic(1, 0.5, 1.0), dial_critic(1, 1.0, 1.0)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), rows, (z, z[::-1].copy()), given_tanh=True)
    got = a.probe("a", N).reshape(-1).astype(np.float64)
    u64 = mean.astype(np.float64); u64[0] += np.float64(np.float32(0.4)) * (1.0 if kind == "Mlp3" else float(np.exp(np.exp(-30.0))))
    assert np.abs(got - np.tanh(u64)).max() <= 4 * 2.0 ** -24, np.abs(got - np.tanh(u64)).max()   # tanhf within 4 ulp of [0.5, 1)
    assert (np.abs(got[3:5]) == CLAMP1).all() and (np.abs(got[1:3]) < CLAMP1).all() and (np.abs(got[5:7]) > CLAMP1).all() and got[7] == 1.0
    compare(a, r64, fig, spec, N, ("tanh", kind))
    # beyond the clamp nothing reaches the mean through atanh: dlogp/dm there is the explicit term plus the Jacobian's, which is 0 too
    a.close()


# ---------------------------------------------------------------------------------------------------------- the Clamp limit
@pytest.mark.parametrize("kind", ["Mlp3", "Mlp2"])
def test_clamp_limit_below_at_inside_at_and_above_the_bounds(B, kind):
    """u below, at, inside, at and above [action_min, action_max] = [-0.5, 0.25] with z = 0 (u = the dialled mean, exactly), and through
    the noise term (rows 5-7: z = 0.1 inside, +-2 outside)"""
    spec = base_spec(kind, action_min=-0.5, action_max=0.25)
    actor, spec.p_units = dial_actor(kind, head2=[0.0])
    mean = np.array([-1.0, -0.5, 0.125, 0.25, 0.75, 0.0, 0.0, 0.0], np.float32)
    z = np.zeros((N, 1), np.float32); z[5:, 0] = [0.125, 2.0, -2.0]
    rows = batch(mean, s_col=np.full(N, -30.0, np.float32))
    crit = [dial_critic(1, 0.5, 1.0), dial_critic(1, -1.0, 1.0)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), rows, (z, z[::-1].copy()))
    got = a.probe("a", N).reshape(-1)
    assert (got[:5] == np.array([-0.5, -0.5, 0.125, 0.25, 0.25], np.float32)).all() and got[6] == 0.25 and got[7] == -0.5
    compare(a, r64, fig, spec, N, ("clamp", kind))
    a.close()


# ---------------------------------------------------------------------------------------------------------- the log-std clamp
def test_log_std_clamp_at_and_beyond_both_bounds_mlp3(B):
    """head2 = [-2, -1, 0, 0.5, 1] with bounds [-1, 0.5]: below, at, inside, at, above.  Beyond the bounds the reference's head2
    gradient is exactly 0; on them it is the inside formula's (closed range)."""
    A = 5
    spec = base_spec("Mlp3", A=A, min_log_std=-1.0, max_log_std=0.5, action_min=-100.0, action_max=100.0)
    actor, spec.p_units = dial_actor("Mlp3", A=A, head2=[-2.0, -1.0, 0.0, 0.5, 1.0])
    rows = batch(np.linspace(-0.8, 0.9, N).astype(np.float32))
    z = spec.draws(N, 3)
    crit = [dial_critic(A, 0.5, 1.0), dial_critic(A, 1.0, 0.5)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), rows, z, A=A)
    g = a.get_params("actor", "grad")[-A:]
    want = r64.probes["actor_grad"][-A:]
    assert want[0] == 0.0 and want[4] == 0.0 and (want[1:4] != 0.0).all()
    assert g[0] == 0.0 and g[4] == 0.0
    compare(a, r64, fig, spec, N, "lstd3")
    a.close()


@pytest.mark.parametrize("lo,hi,s", [
    (0.25, 1.0, [-0.5, 0.0, 1.0, 0.0, 2.0, -0.5, 0.0, 1.0]),       # l = exp(s): inside, AT hi (exp(0) == 1), above
    (1.0, 2.0, [0.0, -1.0, 0.5, 0.0, -2.0, 0.5, 0.0, -1.0]),       # AT lo, below, inside
    (1.0, 2.0, [-1.0] * 8),                                         # every row below: the std head's gradient is exactly 0
])
def test_log_std_clamp_at_and_beyond_both_bounds_mlp2_via_s(B, lo, hi, s):
    spec = base_spec("Mlp2", min_log_std=lo, max_log_std=hi, action_min=-100.0, action_max=100.0)
    actor, spec.p_units = dial_actor("Mlp2")
    rows = batch(np.linspace(-0.8, 0.9, N).astype(np.float32), s_col=np.asarray(s, np.float32))
    z = spec.draws(N, 4)
    crit = [dial_critic(1, 0.5, 1.0), dial_critic(1, 1.0, 0.5)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), rows, z)
    if len(set(s)) == 1:
        H = spec.p_units[-1]
        assert (r64.probes["actor_grad"][-(H + 1):] == 0.0).all() and (a.get_params("actor", "grad")[-(H + 1):] == 0.0).all()
    compare(a, r64, fig, spec, N, ("lstd2", lo))
    a.close()


# ---------------------------------------------------------------------------------------------------------- ties, ReLU at 0, zeros
def test_two_identical_critics_both_pass_the_action_gradient(B):
    """Q_0 == Q_1 = 0.5 a on every row: candle's reduce-min backward is an equality mask, so dq/da = 0.5 + 0.5, not one of them"""
    spec = base_spec("Mlp3", action_min=-100.0, action_max=100.0)
    actor, spec.p_units = dial_actor("Mlp3", head2=[-1.0])
    rows = batch(np.linspace(-0.8, 0.9, N).astype(np.float32))
    crit = [dial_critic(1, 0.5), dial_critic(1, 0.5)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), rows, spec.draws(N, 6))
    assert (r64.probes["dq_da"] == 1.0).all() and (a.probe("dq_da", N) == 1.0).all()
    compare(a, r64, fig, spec, N, "tie")
    a.close()


@pytest.mark.parametrize("relu_out", [False, True])
def test_relu_masks_at_exactly_zero(B, relu_out):
    """a == 0 exactly on rows 0-1 (mean 0, z 0): the dial critic's hidden units relu(a) and relu(-a) sit AT 0, relu'(0) = 0, so
    dq/da is exactly 0 there and 0.5 elsewhere; with an output ReLU, Q = 0.5 a <= 0 passes nothing either"""
    spec = base_spec("Mlp3", action_min=-100.0, action_max=100.0, q_relu_out=relu_out, n_critics=1)
    actor, spec.p_units = dial_actor("Mlp3", head2=[0.0])
    mean = np.array([0.0, 0.0, 0.5, -0.5, 0.25, -0.25, 1.0, -1.0], np.float32)
    z = np.zeros((N, 1), np.float32)
    crit = [dial_critic(1, 0.5)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), batch(mean), (z, z))
    want = np.where(mean == 0.0, 0.0, 0.5) if not relu_out else np.where(mean > 0.0, 0.5, 0.0)
    assert (r64.probes["dq_da"].reshape(-1) == want).all() and (a.probe("dq_da", N).reshape(-1) == want).all()
    compare(a, r64, fig, spec, N, ("relu0", relu_out))
    a.close()


@pytest.mark.parametrize("kind", ["Mlp3", "Mlp2"])
def test_all_zero_networks(B, kind):
    """every parameter 0: mean 0, second output 0 (Mlp2: exp(0) = 1), Q = 0 on every row - all critics tie; every gradient the
    reference has exactly 0 is == 0 on the device (compare() asserts it), the others agree"""
    spec = base_spec(kind, n_critics=3)
    actor = np.zeros(spec.actor_count(), np.float32)
    crit = [const_mlp(O + 1, QU, 1, 0.0, 0.0) for _ in range(3)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), batch(np.linspace(-1, 1, N).astype(np.float32)), spec.draws(N, 8, 0.3))
    assert (a.probe("q_min", N) == 0.0).all() and (a.probe("dq_da", N) == 0.0).all()
    assert (r64.probes["actor_grad"] == 0.0).sum() > 0
    compare(a, r64, fig, spec, N, ("zero", kind))
    a.close()


# ---------------------------------------------------------------------------------------------------------- target, EntCoef
def test_all_rows_terminated_make_the_target_the_reward(B):
    spec = base_spec("Mlp2")
    actor, spec.p_units = dial_actor("Mlp2")
    rows = batch(np.linspace(-0.8, 0.9, N).astype(np.float32), s_col=np.zeros(N, np.float32), term=np.ones(N))
    crit = [dial_critic(1, 0.5, 1.0), dial_critic(1, 1.0, 0.5)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), rows, spec.draws(N, 9, 0.3))
    assert (a.probe("tgt", N) == rows[3]).all() and (r64.probes["tgt"] == rows[3]).all()      # gnd = 0: tgt = r, bit for bit
    compare(a, r64, fig, spec, N, "terminated")
    a.close()


@pytest.mark.parametrize("target_entropy", [50.0, -50.0])
def test_auto_ent_coef_steps_either_way(B, target_entropy):
    """logp + target_entropy of both signs: the first AdamW step from log_alpha = 0 is -lr sign(gradient) up to eps, so alpha rises
    when the policy's entropy is under the target (logp + target > 0) and falls otherwise"""
    lr = 1e-2
    spec = base_spec("Mlp2", ent_coef=("Auto", target_entropy, lr))
    actor, spec.p_units = dial_actor("Mlp2")
    rows = batch(np.linspace(-0.8, 0.9, N).astype(np.float32), s_col=np.zeros(N, np.float32))
    crit = [dial_critic(1, 0.5, 1.0), dial_critic(1, 1.0, 0.5)]
    a, r64, r32, fig = run(B, spec, (actor, crit, [c.copy() for c in crit]), rows, spec.draws(N, 10, 0.3))
    lp = r64.probes["logp"]
    assert ((lp + target_entropy) > 0).all() if target_entropy > 0 else ((lp + target_entropy) < 0).all()
    la = float(a.get_params("log_alpha")[0])
    assert abs(la - np.sign(target_entropy) * lr) < 1e-6 and abs(la - float(r64.params("log_alpha")[0])) < 1e-7   # float32 of +-1e-2: 2^-31
    g = float(a.get_params("log_alpha", "grad")[0])
    assert abs(g - float(r64.probes["log_alpha_grad"][0])) < 1e-5 * abs(g)
    compare(a, r64, fig, spec, N, ("auto", target_entropy))
    a.close()
