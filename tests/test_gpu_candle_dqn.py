"""HIP candle DQN agent (csrc/candle_dqn.hip, through the C ABI) against the committed goldens, the float32 autograd restatement of
border-candle-agent's Dqn and the numpy restatement of its explorer and SmallRng (tests/candle_dqn_restatement.py).

Bars are those of tests/test_gpu_candle_sac.py - probes 1e-4 max-relative, gradients 2e-3, parameters within 0.3 lr, targets 1e-5 -
each max-ed with 4 x the float32-versus-float64 figure of the same restatement on the same inputs (R.f32_f64_figures).  Every
free-running double_dqn case first asserts, on the restatement, that each row's two leading online Q(next_obs) values differ by more
than 1e-4 of the largest |Q| (R.double_dqn_gap): below that the argmax would hang on float32 round-off.  Comparisons between two
acting paths, two agents or two calls are `==` on the raw bits."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import candle_dqn_restatement as R  # noqa: E402
import make_golden_candle_dqn as MG  # noqa: E402
import optimizer_inputs as OI  # noqa: E402

rel = R.rel
ADAMW = MG.ADAMW


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def bar(base, fig):
    return max(base, 4.0 * float(fig))


def _agent(B, spec, bsz, params, **kw):
    a = B.CandleDqn.build(spec.to_config(B, bsz, device=0, **kw))
    a.set_params(params[0], "qnet"); a.set_params(params[1], "qnet_tgt")
    return a


def _close(x, want, tag, tol=5e-4):
    assert abs(x - want) <= tol * abs(want) + 1e-6, (tag, x, want)


def _check_step(a, spec, bsz, want, fig, tag):
    """want: name -> the float32 restatement's value; fig: its f32-vs-f64 figures"""
    for k in ("pred", "q_next", "tgt", "dpred"):
        got = a.probe(k, bsz)
        print(tag, k, rel(got, want[k]), "bar", bar(1e-4, fig[k]))
        assert rel(got, want[k]) < bar(1e-4, fig[k]), (tag, k, rel(got, want[k]), fig[k])            # probes 1e-4, or 4 x fig
    assert (a.probe("y", bsz) == want["y"]).all(), (tag, "y")
    g = a.get_params("qnet", "grad")
    print(tag, "grad", rel(g, want["grad"]), "bar", bar(2e-3, fig["grad"]))
    assert rel(g, want["grad"]) < bar(2e-3, fig["grad"]), (tag, rel(g, want["grad"]))                 # gradients 2e-3, or 4 x fig
    dp = np.abs(a.get_params("qnet") - want["qnet"]).max()
    print(tag, "qnet", dp, "bar", bar(0.3 * spec.lr, fig["qnet"]))
    assert dp < bar(0.3 * spec.lr, fig["qnet"]), (tag, dp)                                            # 0.3 lr, or 4 x fig
    dt = rel(a.get_params("qnet_tgt"), want["qnet_tgt"])
    print(tag, "qnet_tgt", dt, "bar", bar(1e-5, fig["qnet_tgt"]))
    assert dt < bar(1e-5, fig["qnet_tgt"]), (tag, dt)                                                 # targets 1e-5, or 4 x fig


# ---------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_candle_dqn_goldens(B, golden_dir, name):
    spec, bsz, steps, seed = MG.case(name)
    g = np.load(os.path.join(golden_dir, f"candle_dqn_{name}.npz"))
    a = _agent(B, spec, bsz, (g["qnet0"], g["qnet_tgt0"]), record_verbose_level=2)
    for s in range(steps):
        batch = [g[f"s{s}_{k}"] for k in MG.BATCH_KEYS]
        rec = a.update_on_batch(*batch)
        fig = {k: float(g[f"s{s}_fig_{k}"]) for k in R.FIGURE_KEYS}
        for k in R.RECORD_KEYS:
            _close(rec[k], float(g[f"s{s}_{k}"]), (name, s, k), bar(5e-4, 2 * fig["tgt"]))
        want = {k: g[f"s{s}_{k}"] for k in MG.PROBE_KEYS + ("grad", "qnet", "qnet_tgt")}
        _check_step(a, spec, bsz, want, fig, (name, s))
    assert a.n_opts == steps
    a.close()


# ---------------------------------------------------------------------------------------------------------- free runs
def _want(ref):
    w = dict(ref.probes)
    w.update(qnet=ref.params("qnet"), qnet_tgt=ref.params("qnet_tgt"))
    return w


def _free_run(B, spec, bsz, steps, seed, **kw):
    params = spec.init_params(seed)
    a = _agent(B, spec, bsz, params, **kw)
    ref = R.CandleDqnRestatement(spec, *params)
    ref64 = R.CandleDqnRestatement(spec, *params, dtype=torch.float64)
    for s in range(steps):
        batch = R.make_batch(spec, bsz, seed * 100 + s)
        if spec.double_dqn:
            assert R.double_dqn_gap(ref, batch[2]) > 1e-4, ("pick another seed: a near-tie of the online argmax", s, R.double_dqn_gap(ref, batch[2]))
        rec = a.update_on_batch(*batch)
        r = ref.update(*batch)
        ref64.update(*batch)
        fig = R.f32_f64_figures(ref, ref64)
        _close(rec["loss"], r["loss"], (s, "loss"), bar(5e-4, 2 * fig["tgt"]))
        _check_step(a, spec, bsz, _want(ref), fig, (s,))
    assert a.n_opts == steps
    return a, ref


FREE = {
    # examples/gym/dqn_cartpole: obs 4, A 2, [256, 256], B 64, AdamW, Mse
    "cartpole_b64": (R.CandleDqnSpec(4, 2, (256, 256), adamw=ADAMW), 64, 11),
    "cartpole_b64_double": (R.CandleDqnSpec(4, 2, (256, 256), adamw=ADAMW, double_dqn=True), 64, 12),
    # an odd batch over one 32-row block, widths that are no multiple of the 32 / 64 tiles
    "odd_b37_double_smooth_l1": (R.CandleDqnSpec(3, 3, (24, 40), adamw=None, double_dqn=True, critic_loss="SmoothL1"), 37, 13),
    # 33 actions: a second 32-column tile of the last layer; two rows
    "a33_b2": (R.CandleDqnSpec(9, 33, (48, 32), adamw=ADAMW, double_dqn=True), 2, 14),
    # two input k-chunks (obs 70 pads to 128), more rows than one 256-row dW chunk
    "obs70_b300_relu_out": (R.CandleDqnSpec(70, 5, (100, 36), adamw=ADAMW, relu_out=True), 300, 15),
    "b1": (R.CandleDqnSpec(5, 4, (32,), adamw=ADAMW), 1, 16),
    "one_hidden_layer": (R.CandleDqnSpec(6, 3, (48,), adamw=None, soft_update_interval=2, tau=0.25), 16, 17),
    "seven_layers": (R.CandleDqnSpec(6, 3, (32, 24, 32, 24, 32, 24), adamw=ADAMW, double_dqn=True), 16, 18),
}


@pytest.mark.parametrize("name", sorted(FREE))
def test_candle_dqn_free_run_against_the_restatement(B, name):
    spec, bsz, seed = FREE[name]
    a, _ = _free_run(B, spec, bsz, 3, seed)
    a.close()


# ---------------------------------------------------------------------------------------------------------- crafted batches
def _tie_params(spec, seed, cols=(1, 2)):
    """parameters whose output columns `cols` have bit-equal weights and bias, in the online net and in the target"""
    q, t = spec.init_params(seed)
    H = spec.units[-1]
    n_last = spec.n_actions * H + spec.n_actions
    for p in (q, t):
        w = p[-n_last:-spec.n_actions].reshape(spec.n_actions, H)
        b = p[-spec.n_actions:]
        w[cols[1]] = w[cols[0]]; b[cols[1]] = b[cols[0]]
        w[cols[0]] += 0.5; w[cols[1]] += 0.5   # (lift both: the tie is then usually the row's maximum on some rows)
        b[cols[0]] += 1.0; b[cols[1]] += 1.0
    return q, t


@pytest.mark.parametrize("double", (False, True))
def test_ties_resolve_to_the_lower_index_in_the_target_and_in_sample(B, double):
    spec = R.CandleDqnSpec(5, 4, (32,), adamw=ADAMW, double_dqn=double)
    params = _tie_params(spec, 31)
    a = _agent(B, spec, 16, params)
    batch = R.make_batch(spec, 16, 5)
    a.update_on_batch(*batch)
    y = a.probe("y", 16)
    assert (y != 2).all() and (y == 1).any(), y   # column 2 equals column 1 bit for bit: the first maximum is never 2
    # Policy::sample on both acting paths (fresh agents: the update above moved the online columns apart).  The indices come from
    # the DEVICE here - k_cdqn_act on the layer path, the DA_DQN epilogue of k_dense_act on the fused one - and travel through the
    # i64 result copy; numpy's argmax over the device's own Q rows (first maximum) is what they must equal.
    obs = np.random.default_rng(9).standard_normal((64, 5)).astype(np.float32)
    for path in ("layers", "fused"):
        # train mode, epsilon-greedy at eps 0: every call is greedy
        s = _agent(B, spec, 16, params, train=True, explorer=B.EpsilonGreedy(eps_start=0.0, eps_final=0.0, final_step=10))
        s.set_act_path(path)
        q = s.qvalues(obs)
        assert (bits(q[:, 1]) == bits(q[:, 2])).all()
        for n in (64, 33, 1):
            g, info = s.sample(obs[:n], return_info=True)
            assert not info["is_random"]
            assert g.dtype == np.int64 and (g == q[:n].argmax(1)).all() and (g != 2).all(), (path, n, g)
        g = s.sample(obs)
        assert (g == 1).any()
        s.close()
        # eval mode: the 1 % random calls replayed by the restatement's explorer on the same Q rows
        s = _agent(B, spec, 16, params)
        s.set_act_path(path)
        ex = R.CandleDqnExplorer(seed=42)
        greedy_calls = 0
        for _ in range(300):
            g, want = s.sample(obs), ex.sample(q, False)
            assert (g == want).all(), path
            if (want == q.argmax(1)).all():
                greedy_calls += 1
                assert (g != 2).all() and (g == 1).any()
        assert greedy_calls >= 280
        # ... and the raw-row entry point returns the same device indices
        s.set_explorer(B.Softmax(), seed=42)
        ex = R.CandleDqnExplorer(seed=42)
        assert (s.sample_raw(obs) == ex.sample(q, False)).all()
        s.close()
    a.close()


def test_all_terminal_rows_give_the_reward_bit_for_bit(B):
    spec = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW)
    a = _agent(B, spec, 9, spec.init_params(3))
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, 9, 1)
    a.update_on_batch(obs, act, nxt, rew, np.ones(9, np.int8), trunc)
    assert (bits(a.probe("tgt", 9)) == bits(rew)).all()
    a.close()


def test_ignored_fields_change_nothing(B):
    spec = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW, double_dqn=True)
    params = spec.init_params(4)
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, 12, 2)
    rew = 3.0 * rew   # beyond any clip range below
    plain = _agent(B, spec, 12, params)
    other = _agent(B, spec, 12, params, clip_reward=0.5, clip_td_err=(0.0, 0.25))
    for _ in range(2):
        r0 = plain.update_on_batch(obs, act, nxt, rew, term, np.zeros(12, np.int8))
        r1 = other.update_on_batch(obs, act, nxt, rew, term, np.ones(12, np.int8))
    assert r0 == r1
    for k in ("qnet", "qnet_tgt"):
        assert (bits(plain.get_params(k)) == bits(other.get_params(k))).all(), k
    for k in ("pred", "tgt", "dpred"):
        assert (bits(plain.probe(k, 12)) == bits(other.probe(k, 12))).all(), k
    # is_truncated may be left out altogether
    third = _agent(B, spec, 12, params)
    for _ in range(2):
        third.update_on_batch(obs, act, nxt, rew, term)
    assert (bits(plain.get_params("qnet")) == bits(third.get_params("qnet"))).all()
    plain.close(); other.close(); third.close()


def _ring(B, spec, n, seed, per=False, act_shape=(1,), act_dtype=np.int64):
    cfg = B.SimpleReplayBufferConfig(capacity=max(256, n), seed=seed)
    if per:
        cfg.per_config = B.PerConfig()
    rb = B.SimpleReplayBuffer(cfg, (spec.obs_dim,), np.float32, act_shape, act_dtype)
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, n, 70 + seed)
    rb.push(obs, act.reshape((n,) + tuple(act_shape)).astype(act_dtype), nxt, rew, term, trunc)
    return rb


def test_records_at_verbosity_two_and_the_ratio_bookkeeping(B):
    spec = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW)
    params = spec.init_params(6)
    a = _agent(B, spec, 8, params, record_verbose_level=2, train=True, explorer=B.EpsilonGreedy(eps_start=0.0, eps_final=0.0, final_step=10))
    ref = R.CandleDqnRestatement(spec, *params)
    rb = _ring(B, spec, 8, 3)
    obs = np.random.default_rng(1).standard_normal((3, 4)).astype(np.float32)
    for _ in range(5):   # eps 0: every call is greedy, so every call counts as "best"
        _, info = a.sample(obs, return_info=True)
    assert (info["n_samples_act"], info["n_samples_best_act"], info["is_random"]) == (5, 5, False)
    rec = a.opt_with_record(rb)
    twin_rb = _ring(B, spec, 8, 3)
    batch = twin_rb.batch(8)   # a twin ring with the same seed draws the batch the agent's opt drew
    twin_rb.close()
    want = ref.update(batch.obs, batch.act.reshape(-1), batch.next_obs, batch.reward, batch.is_terminated, batch.is_truncated)
    keys = list(R.RECORD_KEYS) + list(ref.param_stats()) + ["ratio_best_act"]
    assert list(rec) == keys, (list(rec), keys)
    for k in R.RECORD_KEYS:
        _close(rec[k], want[k], k)
    for k, v in ref.param_stats().items():
        assert abs(rec[k] - v) < 1e-5 + 1e-4 * abs(v), (k, rec[k], v)
    assert rec["ratio_best_act"] == 1.0
    # the counters were reset: no sample since -> 0
    assert a.opt_with_record(rb)["ratio_best_act"] == 0.0
    # eps 1: random calls are "best" only by chance; with 3 rows of 3 actions some are not
    a.set_explorer(B.EpsilonGreedy(eps_start=1.0, eps_final=1.0, final_step=10), seed=42)
    for _ in range(40):
        _, info = a.sample(obs, return_info=True)
    assert info["n_samples_act"] == 40 and info["n_samples_best_act"] < 40
    ratio = a.opt_with_record(rb)["ratio_best_act"]
    assert ratio == np.float32(info["n_samples_best_act"]) / np.float32(40)
    # verbosity 0: loss and ratio_best_act only, and no best bookkeeping
    b = _agent(B, spec, 8, params, train=True, explorer=B.EpsilonGreedy(eps_start=0.0, eps_final=0.0, final_step=10))
    _, info = b.sample(obs, return_info=True)
    assert info["n_samples_best_act"] == 0
    assert list(b.opt_with_record(rb)) == ["loss", "ratio_best_act"]
    a.close(); b.close(); rb.close()


def test_an_action_index_of_n_actions_is_reported_and_the_parameters_stay(B):
    spec = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW)
    params = spec.init_params(7)
    a = _agent(B, spec, 8, params)
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, 8, 3)
    a.update_on_batch(obs, act, nxt, rew, term, trunc)
    before = {k: a.get_params(k) for k in ("qnet", "qnet_tgt")}
    m0 = a.get_params("qnet", "exp_avg")
    bad = act.copy(); bad[5] = spec.n_actions
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=256, seed=1), (4,), np.float32, (1,), np.int64)
    rb.push(obs, np.full((8, 1), spec.n_actions, np.int64), nxt, rew, term, trunc)
    a.opt(rb)
    with pytest.raises(B.BdrError, match="action index outside"):
        a.sync()
    for k in before:
        assert (bits(a.get_params(k)) == bits(before[k])).all(), k
    assert (bits(a.get_params("qnet", "exp_avg")) == bits(m0)).all()
    with pytest.raises(B.BdrError, match="action index outside"):
        a.update_on_batch(obs, bad, nxt, rew, term, trunc)
    for k in before:
        assert (bits(a.get_params(k)) == bits(before[k])).all(), k
    # the agent goes on: the next valid update takes optimizer step 2, as a twin that never saw the bad batches does
    twin = _agent(B, spec, 8, params)
    twin.update_on_batch(obs, act, nxt, rew, term, trunc)
    twin.update_on_batch(nxt, act, obs, rew, term, trunc)
    a.update_on_batch(nxt, act, obs, rew, term, trunc)
    assert (bits(a.get_params("qnet")) == bits(twin.get_params("qnet"))).all()
    assert a.n_opts == twin.n_opts == 2   # the skipped opts do not count
    a.close(); twin.close(); rb.close()


def test_skipped_updates_in_a_plain_opt_loop_leave_every_counter_where_it_was(B):
    """Agent::opt alone never synchronises: the out-of-range action surfaces through the poll of bdr_agent_opt (every 256 opts).
    Every update enqueued while the word was up was skipped on the device; the Adam step number, n_opts and the soft-update counter
    go back with them, so the agent continues exactly as a twin that never saw the bad ring (soft_update_interval 2: the twin's
    next opt tracks, and so must this agent's)."""
    spec = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW, soft_update_interval=2, tau=0.5)
    params = spec.init_params(7)
    a, twin = _agent(B, spec, 8, params), _agent(B, spec, 8, params)
    good, good2 = _ring(B, spec, 64, 3), _ring(B, spec, 64, 3)
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, 8, 3)
    bad = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=256, seed=1), (4,), np.float32, (1,), np.int64)
    bad.push(obs, np.full((8, 1), -1, np.int64), nxt, rew, term, trunc)
    a.opt(good); twin.opt(good2)
    a.sync()
    before = {k: a.get_params(k) for k in ("qnet", "qnet_tgt")}
    raised = 0
    for k in range(600):
        try:
            a.opt(bad)
        except B.BdrError as e:
            assert "action index outside" in str(e)
            raised = k
            break
    assert 256 <= raised <= 520, raised
    a.sync()
    assert a.n_opts == 1
    for k in before:
        assert (bits(a.get_params(k)) == bits(before[k])).all(), k
    for _ in range(3):
        a.opt(good); twin.opt(good2)
    a.sync(); twin.sync()
    assert a.n_opts == twin.n_opts == 4
    for k in ("qnet", "qnet_tgt"):
        assert (bits(a.get_params(k)) == bits(twin.get_params(k))).all(), k
    for x in (a, twin, good, good2, bad):
        x.close()


def test_n_updates_per_opt_and_the_soft_update_interval_over_a_ring(B):
    """n_updates_per_opt = 3, soft_update_interval = 3 over 7 opts: the target moves after opts 3 and 6 only, by track(tau) of the
    online parameters after the opt's LAST update; the restatement replays the ring's batches"""
    spec = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW, n_updates_per_opt=3, soft_update_interval=3, tau=0.25)
    params = spec.init_params(8)
    a = _agent(B, spec, 8, params)
    ref = R.CandleDqnRestatement(spec, *params)
    rb = _ring(B, spec, 64, 5)
    tgt = [a.get_params("qnet_tgt")]
    for o in range(7):
        a.opt(rb)
        a.sync()
        tgt.append(a.get_params("qnet_tgt"))
        moved = not (bits(tgt[-1]) == bits(tgt[-2])).all()
        assert moved == ((o + 1) % 3 == 0), o
    assert a.n_opts == 7
    # a twin on a twin ring gives the same bits (the schedule is deterministic) ...
    b = _agent(B, spec, 8, params)
    rb2 = _ring(B, spec, 64, 5)
    for o in range(7):
        b.opt(rb2)
    b.sync()
    for k in ("qnet", "qnet_tgt"):
        assert (bits(a.get_params(k)) == bits(b.get_params(k))).all(), k
    # ... and the restatement, fed the batches a third ring with the same seed draws, agrees within the bars after 21 steps
    rb3 = _ring(B, spec, 64, 5)
    for o in range(7):
        bs = [rb3.batch(8) for _ in range(3)]
        ref.opt_([(x.obs, x.act.reshape(-1), x.next_obs, x.reward, x.is_terminated, x.is_truncated) for x in bs])
    dp, dt = np.abs(a.get_params("qnet") - ref.params("qnet")).max(), rel(a.get_params("qnet_tgt"), ref.params("qnet_tgt"))
    print("n_updates_per_opt: qnet", dp, "qnet_tgt", dt)
    assert dp < 0.3 * spec.lr and dt < 1e-5
    for x in (a, b, rb, rb2, rb3):
        x.close()


def test_two_agents_from_the_same_state_give_the_same_bits(B):
    spec = R.CandleDqnSpec(4, 2, (256, 256), adamw=ADAMW, double_dqn=True)
    params = spec.init_params(9)
    a, b = _agent(B, spec, 64, params), _agent(B, spec, 64, params)
    for s in range(3):
        batch = R.make_batch(spec, 64, 40 + s)
        ra, rb_ = a.update_on_batch(*batch), b.update_on_batch(*batch)
        assert ra == rb_
    for k in ("qnet", "qnet_tgt"):
        assert (bits(a.get_params(k)) == bits(b.get_params(k))).all()
    for role in ("grad", "exp_avg", "exp_avg_sq"):
        assert (bits(a.get_params("qnet", role)) == bits(b.get_params("qnet", role))).all()
    a.close(); b.close()


@pytest.mark.parametrize("kind", ("AdamW", "Adam"))
def test_one_optimizer_step_and_the_soft_update_element_by_element(B, kind):
    """adam_element and track_element on the device's OWN gradient (tests/optimizer_inputs.py's adam_f32 / track_f32): exp_avg and
    exp_avg_sq carry the restated bits; a parameter carries the bits of one of the three admitted roots (OI.SQRT_ULPS)"""
    o = OI.Opt("AdamW", 1e-2, 0.8, 0.9, 1e-3, 0.1) if kind == "AdamW" else OI.Opt("Adam", 3e-3)
    spec = R.CandleDqnSpec(5, 3, (24, 16), lr=o.lr, tau=0.3, adamw=dict(beta1=o.b1, beta2=o.b2, eps=o.eps, wd=o.wd) if o.adamw else None)
    params = spec.init_params(10)
    a = _agent(B, spec, 16, params)
    p0, t0 = a.get_params("qnet"), a.get_params("qnet_tgt")
    a.update_on_batch(*R.make_batch(spec, 16, 4))
    g = a.get_params("qnet", "grad")
    assert np.abs(g).max() > 0
    s = OI.scalars_of(o, 1)
    zeros = np.zeros_like(p0)
    forms = [OI.adam_f32(p0, g, zeros, zeros, None, s, u) for u in OI.SQRT_ULPS]
    assert (bits(a.get_params("qnet", "exp_avg")) == bits(forms[0][1])).all()
    assert (bits(a.get_params("qnet", "exp_avg_sq")) == bits(forms[0][2])).all()
    p1 = a.get_params("qnet")
    ok = np.zeros(p1.shape, bool)
    for f in forms:
        ok |= bits(p1) == bits(f[0])
    assert ok.all(), int((~ok).sum())
    assert not (bits(p1) == bits(p0)).all()
    tau32, omt32 = OI.tau_scalars(spec.tau)
    assert (bits(a.get_params("qnet_tgt")) == bits(OI.track_f32(p1, t0, tau32, omt32))).all()
    a.close()


# ---------------------------------------------------------------------------------------------------------- acting
ACT_SPEC = R.CandleDqnSpec(11, 6, (64, 96), adamw=ADAMW)


def _pair(B, spec=ACT_SPEC, seed=21, **kw):
    params = spec.init_params(seed)
    f, l = _agent(B, spec, 4, params, **kw), _agent(B, spec, 4, params, **kw)
    f.set_act_path("fused"); l.set_act_path("layers")
    return f, l, R.CandleDqnRestatement(spec, *params)


def test_the_layer_path_and_k_dense_act_are_bit_equal(B):
    f, l, ref = _pair(B)
    for n in (1, 8, 9, 300):
        obs = np.random.default_rng(n).standard_normal((n, ACT_SPEC.obs_dim)).astype(np.float32)
        qf, ql = f.qvalues(obs), l.qvalues(obs)
        assert qf.shape == (n, 6) and (bits(qf) == bits(ql)).all(), n
        assert np.abs(qf - ref.qvalues(obs)).max() < 1e-5, n
        gf, gl = f.sample(obs), l.sample(obs)   # eval mode: argmax, but for one call in a hundred
        assert (gf == gl).all()
        assert (f.sample_greedy(obs) == qf.argmax(1)).all() and (l.sample_greedy(obs) == qf.argmax(1)).all()
    f.close(); l.close()


@pytest.mark.parametrize("path", ("layers", "fused"))
def test_sample_raw_on_float64_rows_with_a_normaliser(B, path):
    spec = ACT_SPEC
    O = spec.obs_dim
    a = _agent(B, spec, 4, spec.init_params(21))
    twin = _agent(B, spec, 4, spec.init_params(21))
    a.set_act_path(path); twin.set_act_path(path)
    k = np.arange(O)
    mean, std = (0.5 + 0.01 * k).astype(np.float32), (1.0 + 0.125 * (k % 4)).astype(np.float32)
    norm = B.ObsNormalizer(O, 0).set(mean, std)
    for n in (1, 9, 40):
        rows = 0.5 + np.random.default_rng(50 + n).standard_normal((n, O))   # float64
        z = norm.apply(rows.astype(np.float32))
        got = a.sample_raw(rows, norm)
        assert got.dtype == np.int64 and (got == twin.sample(z)).all(), n
        # device rows, dense and strided
        dense = torch.from_numpy(rows).cuda()
        wide = torch.full((n, O + 3), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, :O] = dense
        torch.cuda.synchronize()
        want = twin.sample(z)
        assert (a.sample_raw_device(dense.data_ptr(), n, O * 8, np.float64, norm) == want).all()
        want = twin.sample(z)
        assert (a.sample_raw_device(wide.data_ptr(), n, (O + 3) * 8, np.float64, norm) == want).all()
    a.close(); twin.close(); norm.close()


@pytest.mark.parametrize("path", ("layers", "fused"))
def test_device_rows_dense_and_strided_give_the_host_rows_bits(B, path):
    spec = ACT_SPEC
    O = spec.obs_dim
    a = _agent(B, spec, 4, spec.init_params(21))
    a.set_act_path(path)
    for n in (1, 9, 300):
        obs = np.random.default_rng(60 + n).standard_normal((n, O)).astype(np.float32)
        dense = torch.from_numpy(obs).cuda()
        wide = torch.full((n, O + 5), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, :O] = dense
        torch.cuda.synchronize()
        q = a.qvalues(obs)
        assert (bits(a.qvalues_device(dense.data_ptr(), n, O * 4)) == bits(q)).all()
        assert (bits(a.qvalues_device(wide.data_ptr(), n, (O + 5) * 4)) == bits(q)).all()
        a.set_explorer(B.Softmax(), seed=3); a.train()
        h = a.sample(obs)
        a.set_explorer(B.Softmax(), seed=3)
        d = a.sample_device(wide.data_ptr(), n, (O + 5) * 4)
        assert (h == d).all()
        a.eval()
    a.close()


# ---------------------------------------------------------------------------------------------------------- explorers
@pytest.mark.parametrize("n", (1, 4))
def test_epsilon_greedy_sequence_equals_the_restatement(B, n):
    spec = R.CandleDqnSpec(4, 3, (32,), adamw=ADAMW)
    params = spec.init_params(12)
    a = _agent(B, spec, 4, params, train=True, explorer=B.EpsilonGreedy(eps_start=1.0, eps_final=0.02, final_step=1000))
    obs = np.random.default_rng(2).standard_normal((n, 4)).astype(np.float32)
    q = a.qvalues(obs)
    assert R.double_dqn_gap(R.CandleDqnRestatement(spec, *params), obs) > 1e-4
    ex = R.CandleDqnExplorer("eps_greedy", 1.0, 0.02, 1000, seed=42)
    got, want, eps = [], [], []
    for _ in range(2000):
        w_eps = ex.eps()
        act, info = a.sample(obs, return_info=True)
        got.append(act); want.append(ex.sample(q, True)); eps.append((info["eps"], w_eps))
    assert all(e == w for e, w in eps)
    assert (np.array(got) == np.array(want)).all()
    assert a.explorer_state()["n_opts"] == 2000
    # set_explorer rewinds the stream
    a.set_explorer(B.EpsilonGreedy(eps_start=1.0, eps_final=0.02, final_step=1000), seed=42)
    again = [a.sample(obs) for _ in range(50)]
    assert (np.array(again) == np.array(got[:50])).all()
    a.close()


def test_eval_mode_sequence_equals_the_restatement(B):
    spec = R.CandleDqnSpec(4, 6, (32,), adamw=ADAMW)
    params = spec.init_params(13)
    a = _agent(B, spec, 4, params)
    obs = np.random.default_rng(3).standard_normal((3, 4)).astype(np.float32)
    q = a.qvalues(obs)
    ex = R.CandleDqnExplorer(seed=42)
    got = np.array([a.sample(obs) for _ in range(4000)])
    want = np.array([ex.sample(q, False) for _ in range(4000)])
    assert (got == want).all()
    assert 10 <= int((got != q.argmax(1)).any(1).sum()) <= 80   # about 1 % of the calls took the one random action
    a.close()


@pytest.mark.parametrize("A,seed", [(2, 42), (6, 43), (33, 44)])
def test_softmax_rows_equal_the_restatement_on_the_devices_q_rows(B, A, seed):
    """4096 rows; the restatement is evaluated on the DEVICE's Q rows (qvalues).  A row is left out only when `chosen` lies within
    8 ulp of the total of a cumulative weight - there the host's expf and numpy's exp may part ways - and at most 2 rows may be."""
    spec = R.CandleDqnSpec(5, A, (32,), adamw=ADAMW)
    a = _agent(B, spec, 4, spec.init_params(seed), train=True, explorer_seed=seed)
    obs = (2.0 * np.random.default_rng(seed).standard_normal((4096, 5))).astype(np.float32)
    q = a.qvalues(obs)
    got = a.sample(obs)
    rng = R.SmallRng.seed_from_u64(seed)
    left_out = 0
    for i in range(4096):
        k, cum, total, chosen = rng.weighted_index(R.softmax_row(q[i]), detail=True)
        edges = np.concatenate([cum, [total]]).astype(np.float32)
        near = (np.abs(edges.astype(np.float64) - float(chosen)) <= 8 * np.spacing(edges).astype(np.float64)).any()
        if near:
            left_out += 1
            continue
        assert got[i] == k, (i, got[i], k)
    assert left_out <= 2, left_out
    assert len(set(got.tolist())) == A or A == 33
    a.close()


def test_nan_q_rows_are_refused_by_the_softmax_explorer(B):
    spec = R.CandleDqnSpec(4, 3, (16,), adamw=ADAMW)
    q, t = spec.init_params(14)
    q = q.copy(); q[-1] = np.nan   # the last action's bias
    a = _agent(B, spec, 4, (q, t), train=True)
    with pytest.raises(B.BdrError, match="row 0"):
        a.sample(np.zeros((2, 4), np.float32))
    a.close()


# ---------------------------------------------------------------------------------------------------------- integration
class TableEnv:
    """states 0..7 as one-hot rows; action a moves to (state + a + 1) % 8; reward 1 on reaching state 0; episodes of 6 steps"""
    def __init__(self):
        self.s, self.t, self.acts = 0, 0, []

    def _obs(self):
        o = np.zeros((1, 8), np.float32); o[0, self.s] = 1.0
        return o

    def reset(self, is_done=None):
        self.s, self.t = 3, 0
        return self._obs()

    def reset_with_index(self, ix):
        self.s, self.t = (3 + ix) % 8, 0
        return self._obs()[0]

    def step(self, act):
        a = int(np.asarray(act).reshape(-1)[0])
        assert 0 <= a < 3, a
        self.acts.append(a)
        self.s = (self.s + a + 1) % 8
        self.t += 1
        return self._obs()[0], float(self.s == 0), self.s == 0, self.t == 6 and self.s != 0

    def step_with_reset(self, act):
        import border_amd as B
        obs, r, term, trunc = self.step(act)
        st = B.Step(np.asarray(act), obs.reshape(1, 8), np.array([r], np.float32), np.array([int(term)], np.int8), np.array([int(trunc)], np.int8))
        if st.is_done():
            st.init_obs = self.reset()
        return st


TABLE = R.CandleDqnSpec(8, 3, (32, 32), adamw=ADAMW, soft_update_interval=2)


def test_the_compiled_online_trainer_runs_the_agent_with_integer_actions(B):
    a = _agent(B, TABLE, 16, TABLE.init_params(15), train=True, explorer=B.EpsilonGreedy(eps_start=1.0, eps_final=0.1, final_step=100))
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=256, seed=2), (8,), np.float32, (1,), np.int64)
    env, events = TableEnv(), []
    p0 = a.get_params("qnet")
    st = B.NativeTrainer(B.TrainerConfig(max_opts=30, opt_interval=2, warmup_period=32, record_agent_info_interval=10)).train(
        env, a, rb, (8,), np.float32, on_event=lambda e, o, k, sc: events.append((o, k, sc)))
    a.sync()
    assert st["opt_steps"] == 30 and a.n_opts == 30 and len(env.acts) == st["env_steps"]
    assert set(env.acts) == {0, 1, 2}
    assert not (bits(a.get_params("qnet")) == bits(p0)).all() and np.isfinite(a.get_params("qnet")).all()
    assert len(rb) == min(256, st["env_steps"])
    a.close(); rb.close()


def test_train_offline_the_evaluator_and_model_dir_best(B, tmp_path):
    params = TABLE.init_params(15)
    a, twin = _agent(B, TABLE, 16, params), _agent(B, TABLE, 16, params)
    rb, rb_twin = _ring(B, TABLE, 200, 7), _ring(B, TABLE, 200, 7)
    ev = B.Evaluator(TableEnv(), 3, obs_dim=8, act_dim=1, act_dtype=np.int64)
    events, model_dir = [], str(tmp_path / "model")
    st = B.NativeTrainer(B.TrainerConfig(max_opts=6)).train_offline(a, rb, on_event=lambda e, o, kind, sc: events.append((o, kind, sc)), evaluator=ev,
                                                                    eval_interval=2, save_interval=3, model_dir=model_dir)
    assert st["opt_steps"] == 6
    for o in range(6):
        twin.opt(rb_twin)
    twin.sync()
    for k in ("qnet", "qnet_tgt"):
        assert (bits(a.get_params(k)) == bits(twin.get_params(k))).all(), k
    scores = [sc[0] for o, kind, sc in events if kind == "eval"]
    assert len(scores) == 3 and all(0.0 <= s <= 1.0 for s in scores)
    assert sorted(os.listdir(model_dir)) == ["3", "6", "best"]
    assert sorted(os.listdir(os.path.join(model_dir, "3"))) == ["qnet.pt", "qnet_tgt.pt"]
    last = _agent(B, TABLE, 16, TABLE.init_params(99))
    last.load_params(os.path.join(model_dir, "6"))
    for k in ("qnet", "qnet_tgt"):
        assert (bits(last.get_params(k)) == bits(a.get_params(k))).all(), k
    for x in (a, twin, last, rb, rb_twin):
        x.close()


def test_a_prioritized_ring_is_refused(B):
    a = _agent(B, TABLE, 16, TABLE.init_params(15))
    rb = _ring(B, TABLE, 64, 7, per=True)
    with pytest.raises(B.BdrError, match=r"dqn/base\.rs:135-137"):
        a.opt(rb)
    a.close(); rb.close()


# ---------------------------------------------------------------------------------------------------------- checkpoints
def _write_safetensors(path, tensors):
    import json
    import struct
    hdr, blob = {}, b""
    for name, arr in tensors:
        arr = np.ascontiguousarray(arr, np.float32)
        hdr[name] = {"dtype": "F32", "shape": list(arr.shape), "data_offsets": [len(blob), len(blob) + arr.nbytes]}
        blob += arr.tobytes()
    h = json.dumps(hdr).encode()
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)) + h + blob)


def test_checkpoints(B, tmp_path):
    spec = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW)
    params = spec.init_params(16)
    a = _agent(B, spec, 8, params)
    a.update_on_batch(*R.make_batch(spec, 8, 1))
    d = str(tmp_path / "ck")
    assert [os.path.basename(p) for p in a.save_params(d)] == ["qnet.pt", "qnet_tgt.pt"] == sorted(os.listdir(d))
    b = _agent(B, spec, 8, spec.init_params(98))
    b.load_params(d)
    for k in ("qnet", "qnet_tgt"):
        assert (bits(a.get_params(k)) == bits(b.get_params(k))).all(), k
    # the other format, and the extension fallback: an agent set to *.safetensors loads a directory that holds *.pt only
    d2 = str(tmp_path / "ck2")
    a.set_checkpoint_format("safetensors")
    assert [os.path.basename(p) for p in a.save_params(d2)] == ["qnet.safetensors", "qnet_tgt.safetensors"] == sorted(os.listdir(d2))
    c = _agent(B, spec, 8, spec.init_params(97))
    c.load_params(d2)                      # configured *.pt, only *.safetensors there
    assert (bits(c.get_params("qnet")) == bits(a.get_params("qnet"))).all()
    c2 = _agent(B, spec, 8, spec.init_params(96), ckpt_format="safetensors")
    c2.load_params(d)                      # configured *.safetensors, only *.pt there
    assert (bits(c2.get_params("qnet_tgt")) == bits(a.get_params("qnet_tgt"))).all()
    # a file written elsewhere with the reference's variable names (a candle VarMap: mlp.ln{i}.weight [out][in], mlp.ln{i}.bias)
    d3 = str(tmp_path / "ck3"); os.makedirs(d3)
    rng = np.random.default_rng(5)
    dims = [4, 24, 16, 3]
    for stem in ("qnet", "qnet_tgt"):
        ts = []
        for i in range(3):
            ts.append((f"mlp.ln{i}.bias", rng.standard_normal(dims[i + 1])))     # (any order in the file)
            ts.append((f"mlp.ln{i}.weight", rng.standard_normal((dims[i + 1], dims[i]))))
        _write_safetensors(os.path.join(d3, stem + ".pt"), ts)
        flat = np.concatenate([np.asarray(dict(ts)[f"mlp.ln{i}.{n}"], np.float32).reshape(-1) for i in range(3) for n in ("weight", "bias")])
        b.load_params(d3) if stem == "qnet_tgt" else None
        if stem == "qnet":
            want_q = flat
        else:
            assert (bits(b.get_params("qnet")) == bits(want_q)).all() and (bits(b.get_params("qnet_tgt")) == bits(flat)).all()
    # a missing variable is an error
    _write_safetensors(os.path.join(d3, "qnet.pt"), [("mlp.ln0.weight", np.zeros((24, 4)))])
    with pytest.raises(B.BdrError, match="missing"):
        b.load_params(d3)
    for x in (a, b, c, c2):
        x.close()


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals(B):
    ok = R.CandleDqnSpec(4, 3, (24, 16), adamw=ADAMW)
    with pytest.raises(KeyError):
        B.CandleDqn.build(R.CandleDqnSpec(4, 3, (24,), critic_loss="Huber").to_config(B, 4, device=0))
    c = ok.to_config(B, 4, device=0).to_c()
    import ctypes as C
    h = C.c_void_p()
    L = B._lib.lib()
    c.critic_loss = 7
    assert L.bdr_candle_dqn_create(C.byref(c), C.byref(h)) == 1 and b"critic loss" in L.bdr_last_error()
    c = ok.to_config(B, 4, device=0).to_c(); c.opt.opt_kind = 5
    assert L.bdr_candle_dqn_create(C.byref(c), C.byref(h)) == 1 and b"unknown optimizer" in L.bdr_last_error()
    with pytest.raises(B.BdrError, match="amsgrad"):
        B.CandleDqn.build(R.CandleDqnSpec(4, 3, (24,), adamw=dict(ADAMW, amsgrad=True)).to_config(B, 4, device=0))
    with pytest.raises(B.BdrError, match="n_actions"):
        B.CandleDqn.build(R.CandleDqnSpec(4, 0, (24,)).to_config(B, 4, device=0))
    with pytest.raises(B.BdrError, match="layer width"):
        B.CandleDqn.build(R.CandleDqnSpec(4, 3, (4097,)).to_config(B, 4, device=0))
    with pytest.raises(B.BdrError, match="No device is given"):
        B.CandleDqn.build(ok.to_config(B, 4))
    a = _agent(B, ok, 8, ok.init_params(1))
    rb = _ring(B, ok, 32, 1, act_shape=(1,), act_dtype=np.int32)   # 4-byte action rows
    with pytest.raises(B.BdrError, match="8 bytes"):
        a.opt(rb)
    with pytest.raises(B.BdrError, match="idx_out"):
        B._lib.check(L.bdr_agent_sample_raw(a.handle, None, 1, np.zeros(4, np.float32).ctypes.data_as(C.c_void_p), 0, 0, 0, None, None))
    a.close(); rb.close()


# ---------------------------------------------------------------------------------------------------------- the launch schedule
@pytest.mark.parametrize("double", (False, True))
def test_one_update_takes_at_most_eleven_launches_plus_the_gather(B, double):
    """counted from the profile brackets at the CartPole shape: pack, one forward launch per layer for all passes, k_cdqn_td,
    the input gradients, the grouped dW, reduce + Adam (+ the soft update: interval 1)"""
    spec = R.CandleDqnSpec(4, 2, (256, 256), adamw=ADAMW, double_dqn=double)
    a = _agent(B, spec, 64, spec.init_params(1))
    rb = _ring(B, spec, 200, 1)
    a.opt(rb)
    a.profile_enable(True)
    a.opt(rb)
    a.sync()
    names = [k for k, _ in a.profile_read()]
    a.profile_enable(False)
    assert names == ["sample", "pack", "fwd", "fwd", "fwd", "cdqn_td", "dx", "dx", "dw", "reduce_adam"], names
    assert len(names) - 1 <= 11
    a.close(); rb.close()
