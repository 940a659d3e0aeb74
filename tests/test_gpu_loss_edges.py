"""The loss kernels' clamp, kink and saturation branches on the GPU: every case of tests/edge_inputs.py is run through the Python mirror
(set_params, update_on_batch) and compared with the float64 reference of the same update, in this order: the probes that the dial
construction makes exact, bit for bit; what must be exactly 0; the element-wise quantities at their derived bars; the remaining probes
at the ceilings of the agent's own GPU test file; the losses; every gradient arena as a whole and for its last layer; parameters and
targets at the existing bars (against the committed f32 restatement, their existing reference).  No row is excluded anywhere.

Every figure is printed before it is asserted (pytest -s shows them; LAB.md section 9 holds the maxima measured on an MI355X)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import edge_inputs as E  # noqa: E402


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def _ids(agent):
    return [c.name for c in E.CASES[agent]()]


def _case(agent, name):
    return next(c for c in E.CASES[agent]() if c.name == name)


def _judge(case, got, tag):
    """print every figure, then assert them in the order of E.checks_for"""
    ref = E.run_ref(case, terms=True)
    f32out = E.run_f32(case)
    missing = E.covered(case.coverage(ref))
    assert not missing, (tag, "coverage", missing)
    checks = E.checks_for(case, ref, f32out)
    rows = []
    init = {"param": case.params[0]}     # DQN: entries that no row contributes to stay at their initial value
    for c in checks:
        want = {"f64": ref, "f32": f32out, "init": init}[c.against]
        if c.against == "f32" and c.key not in want:   # only TorchSac lacks keys, and none of a parameter
            raise AssertionError((tag, c.key, "the f32 reference has no such quantity"))
        rows.append((c, c.err(got, want), c.ratio(got, want)))
    for c, err, ratio in rows:
        bar = "elem" if c.kind == "elem" else c.bar
        print(f"EDGE {tag} {c.key} [{c.kind}] err {err:.3g} bar {bar} ratio {ratio:.3g} ({c.how})")
    for c, err, ratio in rows:
        assert ratio <= 1.0, (tag, c.key, c.kind, err, c.bar, c.how)
    for k, v in got.items():
        assert np.isfinite(np.asarray(v, np.float64)).all(), (tag, k, "not finite")


def _candle_got(a, case, rec, probes):
    s, n = case.spec, len(case.batches[-1][0])
    got = dict(rec)
    for k in probes:
        got[k] = a.probe(k, n)
    names = ["actor"] + (["value"] if case.agent == "iql" else [])
    for i in range(s.n_critics):
        names.append(f"critic_{i}")
        got[f"param_critic_tgt_{i}"] = a.get_params(f"critic_tgt_{i}")
    for m in names:
        got[f"grad_{m}"] = a.get_params(m, "grad")
        got[f"param_{m}"] = a.get_params(m)
    return got


# ---------------------------------------------------------------------------------------------------------- IQL
@pytest.mark.parametrize("name", _ids("iql"))
def test_iql_edges(B, name):
    case = _case("iql", name)
    s, n = case.spec, len(case.batches[-1][0])
    a = B.Iql.build(s.to_config(B, n, device=0))
    actor, critics, tgts, value = case.params
    a.set_params(actor, "actor"); a.set_params(value, "value")
    for i in range(s.n_critics):
        a.set_params(critics[i], f"critic_{i}"); a.set_params(tgts[i], f"critic_tgt_{i}")
    for batch in case.batches:
        rec = a.update_on_batch(*batch)
    got = _candle_got(a, case, rec, ("q_tgt_min_value", "v", "u", "tgt", "v_next", "q_pred", "q_tgt_min_actor", "v_obs", "w", "logp"))
    a.close()
    _judge(case, got, ("iql", name))


# ---------------------------------------------------------------------------------------------------------- AWAC
@pytest.mark.parametrize("name", _ids("awac"))
def test_awac_edges(B, name):
    case = _case("awac", name)
    s, n = case.spec, len(case.batches[-1][0])
    a = B.Awac.build(s.to_config(B, n, device=0, **case.build))
    actor, critics, tgts = case.params
    a.set_params(actor, "actor")
    for i in range(s.n_critics):
        a.set_params(critics[i], f"critic_{i}"); a.set_params(tgts[i], f"critic_tgt_{i}")
    for batch in case.batches:
        rec = a.update_on_batch(*batch)
    got = _candle_got(a, case, rec, ("q_data_min", "q_pi_min", "adv", "w", "logp", "act_", "next_act", "next_q", "tgt", "q_pred"))
    a.close()
    _judge(case, got, ("awac", name))


# ---------------------------------------------------------------------------------------------------------- BC
@pytest.mark.parametrize("form", E.BC_FORMS)
@pytest.mark.parametrize("name", _ids("bc"))
def test_bc_edges(B, name, form):
    case = _case("bc", name)
    s, n = case.spec, len(case.batches[-1][0])
    a = B.Bc.build(s.to_config(B, n, device=0, kernel_form=form))
    a.set_params(case.params[0])
    for batch in case.batches:
        rec = a.update_on_batch(*batch)
    got = dict(rec, pred=a.probe("pred", n), dz=a.probe("dz", n), grad=a.get_params(role="grad"), param=a.get_params())
    a.close()
    _judge(case, got, ("bc", name, form))


# ---------------------------------------------------------------------------------------------------------- SAC
# "no_chain": at the 256-wide case the two wide layers run as two launches instead of the chain kernel; at the narrow cases, which the
# chain kernel does not take, it only moves the EntCoef / loss-sum tail back into its kernel (BDR_SAC_TAIL_IN_KERNEL)
SAC_PATHS = {"row_block": {}, "layer_by_layer": {"BDR_NO_SAC_FUSE": "1"}, "no_chain": {"BDR_NO_SAC_CHAIN": "1", "BDR_SAC_TAIL_IN_KERNEL": "1"}}
SAC_ENV = ("BDR_NO_SAC_FUSE", "BDR_NO_SAC_CHAIN", "BDR_SAC_TAIL_IN_KERNEL", "BDR_SAC_CHAIN_TPW", "BDR_SAC_HEADS_FUSE", "BDR_STEP_GRAPH", "BDR_NO_STEP_GRAPH")


def _sac_agent(B, case, n, **kw):
    s = case.spec
    a = B.Sac.build(s.to_config(B, n, device=0, **kw))
    pi, qs, tg = case.params
    a.set_params(pi, "pi")
    for i in range(s.n_critics):
        a.set_params(qs[i], f"qnet_{i}"); a.set_params(tg[i], f"qnet_tgt_{i}")
    return a


@pytest.mark.parametrize("path", sorted(SAC_PATHS))
@pytest.mark.parametrize("name", _ids("sac"))
def test_sac_edges(B, monkeypatch, name, path):
    for k in SAC_ENV: monkeypatch.delenv(k, raising=False)
    for k, v in SAC_PATHS[path].items(): monkeypatch.setenv(k, v)
    case = _case("sac", name)
    s, n = case.spec, len(case.batches[-1][0])
    a = _sac_agent(B, case, n)
    for batch in case.batches:
        rec = a.update_on_batch(*batch)
    got = dict(rec)
    for k in ("q_pred", "q_next", "qvals_min", "next_log_p", "tgt", "q_pi", "log_p", "next_act"):
        got[k] = a.probe(k, n)
    got.update(grad_pi=a.get_params("pi", "grad"), param_pi=a.get_params("pi"), log_alpha=float(a.get_params("log_alpha")[0]))
    for i in range(s.n_critics):
        got[f"grad_q_{i}"], got[f"param_q_{i}"] = a.get_params(f"qnet_{i}", "grad"), a.get_params(f"qnet_{i}")
        got[f"param_q_tgt_{i}"] = a.get_params(f"qnet_tgt_{i}")
    a.close()
    _judge(case, got, ("sac", name, path))


def test_sac_edges_from_the_captured_graph(B, monkeypatch):
    """opt() over a ring that holds the saturating rows of the first SAC case, from the captured graph and from eager launches: the same
    bits, all finite (the eager kernels are the ones test_sac_edges holds against float64)."""
    case = _case("sac", "fix_alpha_eps_default")
    obs, act, nxt, rew, term = case.batches[0][:5]
    outs = []
    for env in ({"BDR_STEP_GRAPH": "1"}, {"BDR_NO_STEP_GRAPH": "1"}):
        for k in SAC_ENV: monkeypatch.delenv(k, raising=False)
        for k, v in env.items(): monkeypatch.setenv(k, v)
        rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=1000, seed=7), (case.spec.obs_dim,), np.float32, (case.spec.act_dim,), np.float32)
        rb.push(obs, act, nxt, rew, term, np.zeros(len(rew), np.int8))
        a = _sac_agent(B, case, 128, seed=5)
        a.train()
        recs = [a.opt_with_record(rb) for _ in range(4)]
        outs.append((recs, [a.get_params(m) for m in ("pi", "qnet_0", "qnet_1", "qnet_tgt_0", "log_alpha")]))
        a.close(); rb.close()
    assert outs[0][0] == outs[1][0], outs
    for x, y in zip(outs[0][1], outs[1][1]):
        assert np.isfinite(x).all() and (x == y).all()
    assert all(np.isfinite(v) for r in outs[0][0] for v in r.values())


# ---------------------------------------------------------------------------------------------------------- DQN
def _dqn_params():
    out = []
    for c in E.CASES["dqn"]():
        n = len(c.batches[-1][3])
        for path in (sorted(E.DQN_PATHS[n]) if c.spec.kind == "mlp" else ["default"]):
            out.append((c.name, path))
    return out


def _dqn_agent(B, case, n):
    a = B.Dqn.build(case.spec.to_config(B, n, device=0))
    a.set_params(case.params[0], "qnet"); a.set_params(case.params[1], "qnet_tgt")
    return a


@pytest.mark.parametrize("name,path", _dqn_params())
def test_dqn_edges(B, monkeypatch, name, path):
    case = _case("dqn", name)
    s, batch = case.spec, case.batches[-1]
    n, A = len(batch[3]), s.n_actions
    for k in E.DQN_ENV: monkeypatch.delenv(k, raising=False)
    for k, v in (E.DQN_PATHS[n][path] if s.kind == "mlp" else {}).items(): monkeypatch.setenv(k, v)
    a = _dqn_agent(B, case, n)
    rec = a.update_on_batch(*batch[:5], **({"weight": batch[5]} if len(batch) > 5 else {}))
    got = dict(loss=rec["loss"], q_pred_all=a.probe("q_pred_all", n * A), q_next_all=a.probe("q_next_all", n * A), pred=a.probe("pred", n),
               tgt=a.probe("tgt", n), grad=a.get_params("grad"), param=a.get_params("qnet"), param_tgt=a.get_params("qnet_tgt"))
    if "td_errs" in rec:
        got["td_errs"] = rec["td_errs"]
    a.close()
    _judge(case, got, ("dqn", name, path))


def test_dqn_edges_through_opt_on_a_per_ring(B, monkeypatch):
    """Agent::opt over a PER ring that holds the rows of the clip case: the tree's samples and weights from the CPU restatement of the
    ring (oracle.PerReplay), the weighted loss from the float64 reference; the restated ring takes the float64 reference's (clipped) TD
    errors as priorities, the device ring the device's own, and the two trees are compared."""
    from oracle.oracle import PerReplay
    for k in E.DQN_ENV: monkeypatch.delenv(k, raising=False)
    case = _case("dqn", "per_huber_clip_b250")
    obs, act, nxt, rew, term, _ = case.batches[0]
    n, cap, bsz = len(rew), 256, 32
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=42, per_config=B.PerConfig(alpha=1.0, normalize="All", n_opts_final=50)),
                              (case.spec.in_dim,), np.float32)
    ring = PerReplay(cap, 42, alpha=1.0, normalize="All", n_opts_final=50)
    rb.push(obs, act.reshape(-1, 1), nxt, rew, term, np.zeros(n, np.int8)); ring.push(n)
    a = _dqn_agent(B, case, bsz)
    ref = E.DqnRef(case.spec, *case.params)
    for step in range(3):
        ixs, ws = ring.batch(bsz)
        r = ref.update(obs[ixs], act[ixs], nxt[ixs], rew[ixs], term[ixs], weight=ws)
        ring.update_priority(ixs, r["td_errs"].astype(np.float32))
        rec = a.opt_with_record(rb)
        print("EDGE per ring step", step, "loss", rec["loss"], "want", float(r["loss"]))
        assert abs(rec["loss"] - float(r["loss"])) <= 1e-4 * abs(float(r["loss"])) + 1e-8, step
        np.testing.assert_allclose(rb.per_tree(), ring.tree.tree(), rtol=2e-4, atol=1e-6)
    a.close(); rb.close()


# ---------------------------------------------------------------------------------------------------------- IQN
@pytest.mark.parametrize("arithmetic", ["bf16x3_6", "f32_exact"])
@pytest.mark.parametrize("name", _ids("iqn"))
def test_iqn_edges(B, name, arithmetic):
    case = _case("iqn", name)
    s, batch = case.spec, case.batches[-1]
    n = len(batch[3])
    a = B.Iqn.build(s.to_config(B, n, device=0, arithmetic=arithmetic))
    a.set_params(case.params[0], "iqn"); a.set_params(case.params[1], "iqn_tgt")
    z_pred, z_tgt = a.forward(batch[0], batch[5], "iqn"), a.forward(batch[2], batch[6], "iqn_tgt")
    rec = a.update_on_batch(*batch)
    got = dict(loss_critic=rec["loss_critic"], z_pred=z_pred, z_tgt=z_tgt, grad=a.get_params("grad"), param=a.get_params("iqn"),
               param_tgt=a.get_params("iqn_tgt"))
    a.close()
    _judge(case, got, ("iqn", name, arithmetic))
