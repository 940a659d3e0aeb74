"""tests/candle_dqn_cnn_restatement.py on the CPU: the goldens regenerate, one row worked by hand in float64 through the head and the
TD step, the bars are what the committed cases give, every committed case meets its ReLU-margin precondition, and each mutation of the
statement moves a compared quantity by at least 10 bars on a committed case."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import candle_dqn_cnn_restatement as R  # noqa: E402
import make_golden_candle_dqn_cnn as MG  # noqa: E402


@functools.lru_cache(maxsize=None)
def _run(i, f64=False):
    c = R.CASES[i]
    r, steps = R.run_case(c, torch.float64 if f64 else torch.float32)
    return R.quantities(c, r, steps)


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_the_goldens_regenerate(i):
    c = R.CASES[i]
    gold = np.load(MG.path_of(c))
    new = MG.golden_of(c)
    assert sorted(gold.files) == sorted(new)
    for k in gold.files:
        a, b = np.asarray(gold[k]), np.asarray(new[k])
        if a.dtype.kind in "iu":
            assert (a == b).all(), k
        else:   # (another BLAS or thread count moves the last bits of a float32 evaluation: the quantity's own bar - what the device's
            # accumulation order is allowed - relative to its largest entry)
            kind = k.split("/")[0].replace("grad_norm:", "grad:").replace("grad_sample:", "grad:").split("_sample")[0]
            assert np.abs(a.astype(np.float64) - b).max() <= R.BAR[kind] * max(np.abs(a).max(), 1e-30) + (1e-9 if kind == "qnet" else 0), k
    assert os.path.getsize(MG.path_of(c)) < 64 * 1024


def test_the_bars_are_what_the_committed_cases_give():
    got = {}
    for i, c in enumerate(R.CASES):
        q32, q64 = _run(i), _run(i, True)
        for name in q32:
            k = R.kind_of(name)
            got[k] = max(got.get(k, 0.0), R.distance(k, q32[name], q64[name]))
    assert sorted(got) == sorted(R.F32_F64)
    for k, v in got.items():
        print(k, v, R.F32_F64[k])
        assert R.F32_F64[k] / R.DRIFT <= v <= R.F32_F64[k] * R.DRIFT, (k, v, R.F32_F64[k])
        assert R.BAR[k] == 4.0 * R.F32_F64[k]


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_every_committed_case_meets_the_relu_margin_precondition(i):
    pre = R.precondition(R.CASES[i])
    print(R.CASES[i].name, pre)
    assert sorted(pre) == ["argmax", "c1", "c2", "c3", "l1"]
    assert min(pre.values()) > 1.0, pre


def test_one_row_by_hand_in_float64_through_the_head_and_the_td_step():
    """the trunk's features are taken from the restatement; l1, ReLU, l2, the gather, the maximum over the target's row, the target,
    the loss and dLoss/dpred are written out in numpy float64"""
    c = R.CASES[2]   # B = 1, two actions, Mse, the exact tie
    qnet, qnet_tgt, batches = R.case_inputs(c)
    obs, act, nxt, rew, term, _ = batches[0]
    r = R.CandleDqnCnnRestatement(c.spec, qnet, qnet_tgt, torch.float64)
    sl = R.var_slices(c.spec.n_stack, c.spec.n_actions)

    def head(flat, net, rows):
        z3 = r.pre_activations(net, rows)[2][0]                              # [64][7][7]
        f = np.maximum(z3, 0).reshape(-1)                                     # (c, h, w)
        w4, b4 = flat[sl["l1.weight"]].astype(np.float64).reshape(512, 3136), flat[sl["l1.bias"]].astype(np.float64)
        w5, b5 = flat[sl["l2.weight"]].astype(np.float64).reshape(-1, 512), flat[sl["l2.bias"]].astype(np.float64)
        return w5 @ np.maximum(w4 @ f + b4, 0) + b5
    q_o, q_t = head(qnet, r.qnet, obs), head(qnet_tgt, r.qnet_tgt, nxt)
    assert q_t[0] == q_t[1]
    pred, y = q_o[act[0]], int(np.argmax(q_t))
    tgt = float(rew[0]) + ((1.0 - float(term[0])) * float(np.float32(c.spec.gamma))) * q_t[y]
    rec = r.update(*batches[0])
    assert y == 0 == int(r.probes["y"][0])
    assert abs(r.probes["pred"][0] - pred) < 1e-12 and abs(r.probes["tgt"][0] - tgt) < 1e-12
    assert term[0] == 1 and tgt == float(rew[0])
    assert abs(rec["loss"] - (pred - tgt) ** 2) < 1e-12 and abs(r.probes["dpred"][0] - 2 * (pred - tgt)) < 1e-12


def _moves(i, kinds, **mutation):
    """the largest distance / bar over the named quantity kinds between the float32 statement and its mutation on case i"""
    c = R.CASES[i]
    want = _run(i)
    got = R.quantities(c, *R.run_case(c, **mutation))
    return max(R.distance(R.kind_of(q), got[q], want[q]) / R.BAR[R.kind_of(q)] for q in want if R.kind_of(q) in kinds)


@pytest.mark.parametrize("mutation", ("no_div255", "hwc_flatten", "no_relu3"))
def test_a_mutated_network_moves_the_prediction_by_ten_bars(mutation):
    m = _moves(0, ("pred", "grad:l1.weight"), **{mutation: True})
    print(mutation, m)
    assert m >= 10.0


class _TargetFromOnline(R.CandleDqnCnnRestatement):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.qnet_tgt = self.qnet


class _CountsUpdates(R.CandleDqnCnnRestatement):
    def opt_(self, batches):
        rec = {}
        for b in batches:
            rec = self.update_critic(*b)
            self.soft_update_counter += 1
            if self.soft_update_counter == self.spec.soft_update_interval:
                self.soft_update_counter = 0
                self.track(self.spec.tau)
        self.n_opts += 1
        return rec


def _with(cls, c):
    qnet, qnet_tgt, batches = R.case_inputs(c)
    r = cls(c.spec, qnet, qnet_tgt)
    steps = []
    for b in batches:
        rec = r.update(*b)
        steps.append(dict(loss=rec["loss"], **{k: np.array(v) for k, v in r.probes.items()}))
    return R.quantities(c, r, steps)


def test_a_target_from_the_online_net_moves_the_target_by_ten_bars():
    want, got = _run(0), _with(_TargetFromOnline, R.CASES[0])
    m = R.distance("tgt", got["tgt/0"], want["tgt/0"]) / R.BAR["tgt"]
    print(m)
    assert m >= 10.0


def test_a_soft_update_counted_in_updates_moves_the_target_parameters_by_ten_bars():
    """n_updates_per_opt = 2 with soft_update_interval = 2 on the first committed case's inputs: counted in opts the target is
    untouched after one opt, counted in updates it has tracked once"""
    c = R.CASES[0]
    spec = R.CandleDqnCnnSpec(**{**c.spec.__dict__, "n_updates_per_opt": 2, "soft_update_interval": 2, "tau": 0.25})
    qnet, qnet_tgt, batches = R.case_inputs(c)
    a, b = R.CandleDqnCnnRestatement(spec, qnet, qnet_tgt), _CountsUpdates(spec, qnet, qnet_tgt)
    a.opt_(batches[:2]); b.opt_(batches[:2])
    assert (a.params("qnet_tgt") == qnet_tgt).all()
    m = R.distance("qnet_tgt", b.params("qnet_tgt"), a.params("qnet_tgt")) / R.BAR["qnet_tgt"]
    print(m)
    assert m >= 10.0
