"""The candle DQN CNN group on the GPU (csrc/candle_dqn_cnn_group.hpp, csrc/conv_group.hpp): P members stepped by the 17 launches of
one member against P twins stepped alone, bit for bit; member 1 of a group of three as a committed case of
tests/candle_dqn_cnn_restatement.py against its float64 run under the module's own bars (R.BAR); a poisoned member; the plan; the
refusals that need a device."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import candle_dqn_cnn_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
ROUNDS = 3
# name: (n_stack, actions, batch, double_dqn, critic_loss, AdamW?)
SHAPES = {"b3_ns1_a18": (1, 18, 3, True, "SmoothL1", False),    # three instances; M = 243 / 147 rows, ragged in the 64-row tiles
          "b8_ns4_a6": (4, 6, 8, False, "Mse", True),
          "b33_ns4_a2": (4, 2, 33, False, "Mse", True)}         # one image past a 32-row head tile


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def spec_of(name, i):
    """member i of a shape: its own learning rate, optimizer scalars, discount, tau and soft_update_interval (1 and 2)"""
    ns, A, _b, dd, loss, adamw = SHAPES[name]
    opt = dict(beta1=0.9 - 0.05 * i, beta2=0.999 - 0.01 * i, eps=1e-8 * (i + 1), wd=0.01 * (i + 1)) if adamw else None
    return R.CandleDqnCnnSpec(ns, A, lr=1e-4 * (i + 1), adamw=opt, gamma=0.99 - 0.02 * i, tau=0.1 + 0.2 * i, soft_update_interval=1 + i % 2, double_dqn=dd,
                              critic_loss=loss)


@functools.lru_cache(maxsize=None)
def inputs(name, i):
    """(qnet, qnet_tgt) and the 16 ring rows of member i"""
    s = spec_of(name, i)
    return s.init_params(500 + i), R.make_batch(s, 16, 600 + i)


def build(B, name, i, verbose):
    s = spec_of(name, i)
    return s.to_config(B, SHAPES[name][2], device=0, seed=i, record_verbose_level=2 if verbose else 0)


def ring(B, name, i, seed, data=None):
    s = spec_of(name, i)
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=seed), (s.row_bytes,), np.uint8, (1,), np.int64)
    obs, act, nxt, rew, term, trunc = data or inputs(name, i)[1]
    rb.push(obs, act.reshape(-1, 1), nxt, rew, term, trunc)
    return rb


def load(a, name, i):
    p = inputs(name, i)[0]
    a.set_params(p[0], "qnet"); a.set_params(p[1], "qnet_tgt")


def state(a, n):
    out = {k: a.get_params(k).tobytes() for k in ("qnet", "qnet_tgt")}
    for role in ("exp_avg", "exp_avg_sq", "grad"):
        out[role] = a.get_params("qnet", role).tobytes()
    for key in R.PROBE_KEYS + ("y",):
        out[key] = a.probe(key, n).tobytes()
    out["n_opts"] = a.n_opts
    return out


def rec_bits(rec):
    return [(k, np.float32(v).view(np.uint32)) for k, v in rec.items()]


@functools.lru_cache(maxsize=None)
def twin(name, i, data_of=None):
    """member i stepped alone for ROUNDS opts over its own ring (data_of: over member data_of's rows, what a view reads)"""
    import border_amd as B
    a = B.CandleDqn.build(build(B, name, i, i % 2 == 1))
    load(a, name, i)
    rb = ring(B, name, i, 100 + i, inputs(name, data_of)[1] if data_of is not None else None)
    for k in range(ROUNDS):
        rec = a.opt_with_record(rb) if k == ROUNDS - 1 else a.opt(rb)
    a.sync()
    out = (state(a, SHAPES[name][2]), rec)
    a.close(); rb.close()
    return out


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_rounds_equal_the_members_stepped_alone(B, name, P):
    """rings of their own for P = 1, views of ONE ring for P = 3"""
    g = B.CandleDqnCnnGroup.build([build(B, name, i, i % 2 == 1) for i in range(P)])
    for i in range(P): load(g.members[i], name, i)
    owner = ring(B, name, 0, 999) if P > 1 else None
    bufs = [owner.view(100 + i) for i in range(P)] if owner else [ring(B, name, 0, 100)]
    assert g.form == "candle_dqn_cnn_layers" and g.launches_per_round == 17 and len(g) == P
    base = g.kernel_launches
    for k in range(ROUNDS):
        recs = g.opt_with_record(bufs) if k == ROUNDS - 1 else g.opt(bufs)
    assert g.kernel_launches - base == 17 * ROUNDS
    g.sync()
    for i in range(P):
        want, want_rec = twin(name, i, 0 if owner else None)
        got = state(g.members[i], SHAPES[name][2])
        for k in want:
            assert got[k] == want[k], (name, P, i, k)
        assert rec_bits(recs[i]) == rec_bits(want_rec), (name, P, i)
    assert len({state(m, SHAPES[name][2])["qnet"] for m in g.members}) == P   # the members differ: a swapped table entry cannot pass
    g.close()
    for rb in bufs: rb.close()
    if owner: owner.close()


@pytest.mark.parametrize("case", [c for c in R.CASES if c.batch > 1], ids=lambda c: c.name)
def test_member_one_is_a_committed_case_against_float64(B, case):
    """member 1 carries the committed case's spec and parameters (R.case_inputs) between two members with other parameters; its ring
    holds the case's rows, and a twin ring of the same seed names the batches the round drew.  Every compared quantity of the case
    (probes, loss, the ten gradients, parameters, target parameters) against the float64 restatement on those batches, under R.BAR."""
    qnet, qnet_tgt, batches = R.case_inputs(case)
    rows = tuple(np.concatenate([b[k] for b in batches]) for k in range(6))
    cfgs = [case.spec.to_config(B, case.batch, device=0, seed=i) for i in range(3)]
    g = B.CandleDqnCnnGroup.build(cfgs)
    for i, m in enumerate(g.members):
        p = (qnet, qnet_tgt) if i == 1 else case.spec.init_params(40 + i)
        m.set_params(p[0], "qnet"); m.set_params(p[1], "qnet_tgt")
    mk = lambda seed: B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=seed), (case.spec.row_bytes,), np.uint8, (1,), np.int64)
    bufs, shadow = [mk(70 + i) for i in range(3)], mk(71)
    for rb in bufs + [shadow]:
        rb.push(rows[0], rows[1].reshape(-1, 1), *rows[2:])
    ref = R.CandleDqnCnnRestatement(case.spec, qnet, qnet_tgt, torch.float64)
    sl = R.var_slices(case.spec.n_stack, case.spec.n_actions)
    worst = {}
    for k in range(case.n_updates):
        g.opt(bufs); g.sync()
        x = shadow.batch(case.batch)
        rec = ref.update(x.obs, x.act.reshape(-1), x.next_obs, x.reward, x.is_terminated, x.is_truncated)
        m = g.members[1]
        assert (m.probe("y", case.batch) == ref.probes["y"]).all(), k
        got = {key: m.probe(key, case.batch) for key in R.PROBE_KEYS}
        want = {key: np.asarray(ref.probes[key]) for key in R.PROBE_KEYS}
        gr = m.get_params("qnet", "grad")
        for v in R.VAR_NAMES:
            got["grad:" + v], want["grad:" + v] = gr[sl[v]], np.asarray(ref.probes["grad"])[sl[v]]
        for key in got:
            worst[key] = max(worst.get(key, 0.0), R.distance(key, got[key], want[key]))
    for which in ("qnet", "qnet_tgt"):
        worst[which] = R.distance(which, g.members[1].get_params(which), ref.params(which))
    for key, d in worst.items():
        print(case.name, key, d, "bar", R.BAR[key])
    for key, d in worst.items():
        assert d < R.BAR[key], (case.name, key, d, R.BAR[key])
    g.close()
    for rb in bufs + [shadow]: rb.close()


def test_a_poisoned_member_is_untouched_reported_and_rolled_back(B):
    name, P, bad = "b3_ns1_a18", 3, 1
    g = B.CandleDqnCnnGroup.build([build(B, name, i, False) for i in range(P)])
    twins = [B.CandleDqn.build(build(B, name, i, False)) for i in range(P)]
    for i in range(P): load(g.members[i], name, i); load(twins[i], name, i)
    before = state(g.members[bad], 3) if False else {k: g.members[bad].get_params(k).tobytes() for k in ("qnet", "qnet_tgt")}
    data = [inputs(name, i)[1] for i in range(P)]
    data[bad] = (data[bad][0], np.full(16, SHAPES[name][1], np.int64)) + data[bad][2:]   # every action out of range
    bufs = [ring(B, name, i, 100 + i, data[i]) for i in range(P)]
    tbufs = [ring(B, name, i, 100 + i, data[i]) for i in range(P)]
    for _ in range(2):
        g.opt(bufs)
        for i in range(P): twins[i].opt(tbufs[i])
    with pytest.raises(B.BdrError, match=r"member 1: .*action index outside"):
        g.sync()
    g.sync()   # reported once
    for i in range(P):
        if i == bad:
            with pytest.raises(B.BdrError, match="action index outside"):
                twins[i].sync()
            assert g.members[i].n_opts == twins[i].n_opts == 0
            for k in before:
                assert g.members[i].get_params(k).tobytes() == before[k], k
            assert not np.frombuffer(g.members[i].get_params("qnet", "exp_avg").tobytes(), np.float32).any()
        else:
            twins[i].sync()
            assert g.members[i].n_opts == twins[i].n_opts == 2
            assert state(g.members[i], 3) == state(twins[i], 3), i
    g.close()
    for x in twins + bufs + tbufs: x.close()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("P", [1, 3])
def test_the_plan_has_seventeen_launches(B, P, double):
    s = R.CandleDqnCnnSpec(1, 3, adamw=ADAMW, double_dqn=double)
    g = B.CandleDqnCnnGroup.build([s.to_config(B, 2, device=0, seed=i) for i in range(P)])
    assert g.launches_per_round == 17 and g.form == "candle_dqn_cnn_layers" and g.info()["n_members"] == P
    g.close()


def test_refusals_that_need_a_device(B):
    from border_amd.iql import CandleMlpConfig
    s = R.CandleDqnCnnSpec(1, 3, adamw=ADAMW)
    ok = lambda i: B.CandleDqn.build(s.to_config(B, 2, device=0, seed=i))
    cases = {
        "not a candle DQN agent with the AtariCnn": lambda: B.CandleDqn.build(B.CandleDqnConfig(
            obs_dim=4, n_actions=2, model_config=B.CandleDqnModelConfig(CandleMlpConfig((64,))), batch_size=2, device=0)),
        "shape": lambda: B.CandleDqn.build(R.CandleDqnCnnSpec(1, 4, adamw=ADAMW).to_config(B, 2, device=0)),
        "n_updates_per_opt": lambda: B.CandleDqn.build(R.CandleDqnCnnSpec(1, 3, adamw=ADAMW, n_updates_per_opt=2).to_config(B, 2, device=0)),
    }
    rb = ring(B, "b3_ns1_a18", 0, 5, R.make_batch(s, 8, 1))
    for text, make in cases.items():
        other, a, b = make(), ok(0), ok(2)
        with pytest.raises(B.BdrError, match=r"member 1 cannot join a candle DQN CNN group.*" + text):
            B.CandleDqnCnnGroup([a, other, b])
        a.opt(rb); b.opt(rb); a.sync(); b.sync()          # nobody was adopted: every agent still steps alone
        assert a.n_opts == b.n_opts == 1
        if text != "not a candle DQN agent with the AtariCnn":
            other.opt(rb); other.sync()
            assert other.n_opts == 1
        for x in (a, b, other): x.close()
    g = B.CandleDqnCnnGroup.build([s.to_config(B, 2, device=0, seed=i) for i in range(2)])
    store = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=11, frame_stack=1), (s.row_bytes,), np.uint8, (1,), np.int64)
    rb2 = ring(B, "b3_ns1_a18", 0, 6, R.make_batch(s, 8, 1))
    launches = g.kernel_launches
    for call in (g.opt, g.opt_with_record):
        with pytest.raises(B.BdrError, match="member 1: a frame-stack store"):
            call([rb, store])
    assert g.kernel_launches == launches
    g.opt([rb, rb2]); g.sync()
    assert [m.n_opts for m in g.members] == [1, 1]
    g.close()
    for x in (rb, rb2, store): x.close()
