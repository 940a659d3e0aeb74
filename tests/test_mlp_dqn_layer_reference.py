"""Host checks of tests/mlp_dqn_layer_reference.py (no GPU): the f64 reference against f64 torch autograd of a plain DQN step, the
sequential-f32 restatement against criteria (a) to (c) and the stored RESTATEMENT_RATIO, every case's path, geometry and branch states
from its inputs, and every mutant rejected."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_dqn_layer_reference as X  # noqa: E402

RUNS = [(c, step, env) for c in X.CASES.values() for env in (((), (("BDR_NO_MLP_LDS", "1"),)) if c.one_wg else ((),)) for step in range(len(c.batches))]
IDS = ["%s%s-%d" % (c.name, "-global" if env else "", c.batches[step]) for c, step, env in RUNS]
_inp = {}


def host(c, step, env=()):
    k = (c.name, step, env)
    if k not in _inp: _inp[k] = X.host_inputs(c, step, env=env)
    return _inp[k]


def torch_step(c, B, step):
    """a plain DQN step in f64 autograd on the unpadded numbers: activations of every instance, per-row values, gradients"""
    q, qt = X.case_params(c)
    obs, act, nobs, rew, term, w = X.case_batch(c, B, step)
    t = lambda x: torch.from_numpy(np.asarray(x, np.float64))

    def params(flat):
        out, o = [], 0
        for s in X.shapes(c):
            n = int(np.prod(s)); out.append(t(flat[o:o + n]).reshape(s).clone().requires_grad_(True)); o += n
        return out

    def net(p, x):
        hs = []
        for l in range(c.L):
            x = x @ p[2 * l].T + p[2 * l + 1]
            if l < c.L - 1 or c.act_out: x = torch.relu(x)
            hs.append(x)
        return hs
    P, PT = params(q), params(qt)
    h0 = net(P, t(obs))
    with torch.no_grad():
        h1 = net(PT, t(nobs))
        h2 = net(P, t(nobs)) if c.double else None
        idx = (h2 if c.double else h1)[-1].argmax(1)
        tgt = t(rew) + (1 - t(term)) * X.f32(X.GAMMA) * h1[-1].gather(1, idx[:, None])[:, 0]
    pred = h0[-1].gather(1, torch.from_numpy(act)[:, None])[:, 0]
    fn = torch.nn.functional.smooth_l1_loss if c.loss == "SmoothL1" else torch.nn.functional.mse_loss
    if w is None:
        loss = fn(pred, tgt)
    else:
        x = t(w) * (pred - tgt).abs().clip(X.f32(c.clip[0]), X.f32(c.clip[1]))
        loss = fn(x, torch.zeros_like(x))
    loss.backward()
    return h0, h1, h2, pred, tgt, loss, P


@pytest.mark.parametrize("c,step,env", [r for r in RUNS if not r[2]], ids=[i for i, r in zip(IDS, RUNS) if not r[2]])
def test_f64_reference_equals_autograd(c, step, env):
    B = c.batches[step]
    inp = X.host_inputs(c, step, dtype=np.float64)
    ops = X.reference(inp)
    h0, h1, h2, pred, tgt, loss, P = torch_step(c, B, step)
    lay = X.layers(c)
    close = lambda a, b, what: np.testing.assert_allclose(np.asarray(a), b.detach().numpy(), rtol=1e-11, atol=1e-12, err_msg=what)
    for z, hs in enumerate([h0, h1, h2][:c.nz]):
        for l in range(c.L):
            close(ops["z%d.h%d" % (z, l)].ref[:, :lay[l][1]], hs[l], "z%d.h%d" % (z, l))
    close(inp["pred"], pred, "pred"); close(inp["tgt"], tgt, "tgt"); close(inp["loss"][0], loss, "loss")
    for l, (i, o, kp, np_, _) in enumerate(lay):
        g = ops["gW%d.sum" % l if inp["chunks"] else "gW%d" % l].ref
        close(g[:kp * np_].reshape(kp, np_)[:i, :o].T, P[2 * l].grad, "gW%d" % l)
        close(g[kp * np_:][:o], P[2 * l + 1].grad, "gb%d" % l)
        assert not g[:kp * np_].reshape(kp, np_)[i:].any() and not g[:kp * np_].reshape(kp, np_)[:, o:].any() and not g[kp * np_:][o:].any()


def test_restatement_passes_and_reproduces_the_stored_ratios():
    worst = {}
    for c, step, env in RUNS:
        inp = host(c, step, env)
        ops, dev = X.reference(inp), X.restatement(inp)
        bad = X.failures(ops, X.exact(inp), dev) + X.padding_failures(inp)
        assert not bad, (c.name, step, bad)
        for k, v in X.ratios(ops, dev).items(): worst[k] = max(worst.get(k, 0.0), v)
    assert set(worst) == set(X.RESTATEMENT_RATIO), sorted(set(worst) ^ set(X.RESTATEMENT_RATIO))
    for k, v in worst.items():
        assert abs(v - X.RESTATEMENT_RATIO[k]) < 6e-4, (k, v, X.RESTATEMENT_RATIO[k])
        assert X.LAMBDA[k] == max(1.0, 4.0 * X.RESTATEMENT_RATIO[k])


FORM = {   # the step every update takes by default, written out (the one-workgroup cases take "global" with BDR_NO_MLP_LDS=1)
    "c1-double": ("lds",), "two-blocks": ("global",), "ragged-lds": ("lds",), "ragged-deep": ("lds",), "one-row": ("lds",), "wide-in": ("lds",),
    "wide-hidden": ("lds",), "a64-double": ("lds",), "l-65": ("layers_head",), "l-65-double": ("layers_head",), "l-wide-head": ("layers_td",),
    "l-wide-head-fused": ("layers_head",), "l-a33": ("layers_td",), "l-a64-double": ("layers_td",), "l-chunks": ("layers_head", "layers_head", "lds"),
    "l-chunks-layers": ("layers_head",) * 3, "l-deep": ("layers_head",), "l-wide-k": ("layers_head",), "l-big-tiles": ("tiles",),
}


def test_every_case_takes_the_step_it_is_there_for():
    assert set(FORM) == set(X.CASES)
    for c in X.CASES.values():
        for step, B in enumerate(c.batches):
            assert X.predict_form(c, B) == FORM[c.name][step], (c.name, B)
            if c.one_wg: assert X.predict_form(c, B, (("BDR_NO_MLP_LDS", "1"),)) == "global"
    C = X.CASES
    assert X.lds_bytes(C["two-blocks"], 64) == 0 and 4 * 9 * 64 * 68 == 156672 > 150 * 1024          # the plan that does not fit
    assert X.lds_bytes(C["ragged-lds"], 48) == 4 * 9 * 48 * 68 <= 150 * 1024
    assert X.predict_form(C["l-65"], 65, (("BDR_NO_MLP_HEAD_FUSE", "1"),)) == "layers_td"
    # row blocks
    assert 48 % 32 == 16 and 33 % 32 == 1 and 65 % 32 == 1 and C["ragged-deep"].L == 4 and C["l-deep"].L == 9 == 8 + 1
    lay = X.layers(C["wide-in"]); assert lay[0][2] == 128 and C["wide-in"].A > 32
    lay = X.layers(C["wide-hidden"]); assert (lay[1][2] // 32) * (lay[1][3] // 32) + 1 * (lay[1][2] // 32) == 12 > 8
    assert X.layers(C["l-wide-k"])[1][2] == 512 and X.layers(C["l-a33"])[0][3] == 128 and C["a64-double"].A == 64 == C["l-a64-double"].A
    assert X.layers(C["l-wide-head"])[2][2] == 192 > 128
    # row chunks of the grouped weight gradient
    for name in ("l-chunks", "l-chunks-layers"):
        c = C[name]
        assert X.predict_chunks(c, 515, "layers_head") == 2 and X.dw_rows(515, 2) == [(0, 288), (288, 515)] and (515 - 288) % 32 == 3
        assert X.predict_chunks(c, 4100, "layers_head") == 16
        rows = X.dw_rows(4100, 16)
        assert rows[0] == (0, 288) and rows[14] == (4032, 4100) and rows[15][0] >= rows[15][1]           # chunk 15 is empty
    assert X.predict_chunks(C["l-chunks-layers"], 40, "layers_head") == 1 < 16 and X.predict_chunks(C["l-chunks"], 40, "lds") == 0
    assert {c.loss for c in C.values()} == {"Mse", "SmoothL1"}
    assert {c.loss for c in C.values() if c.one_wg} == {"Mse", "SmoothL1"} == {c.loss for c in C.values() if not c.one_wg}


@pytest.mark.parametrize("c,step,env", [r for r in RUNS if not r[2]], ids=[i for i, r in zip(IDS, RUNS) if not r[2]])
def test_branch_states_of_the_inputs(c, step, env):
    inp = host(c, step)
    B, L = inp["B"], c.L
    act = inp["act"]
    if c.A > 1: assert (act != 0).all(), "action 0 has a row"
    if B >= 33: assert np.bincount(act, minlength=c.A).max() >= 17
    assert not inp["dy"][L - 1][:, 0].any() or c.A == 1
    if B >= 17:
        for l in range(L - 1):
            v = inp["acts"][0][l][:, :X.layers(c)[l][1]]
            assert (v > 0).any() and (v == 0).any(), "one ReLU state only in layer %d" % l
    if c.special == "all-terminal":
        assert (inp["term"] == 1).all() and np.array_equal(X.bits(inp["tgt"]), X.bits(inp["reward"]))
    else:
        assert B == 1 or ((inp["term"] == 0).any() and (inp["term"] == 1).any())
    if c.weighted:
        raw = np.abs(inp["pred"] - inp["tgt"])
        lo, hi = np.float32(c.clip[0]), np.float32(c.clip[1])
        assert (raw < lo).any() and ((raw >= lo) & (raw <= hi)).any() and (raw > hi).any(), "not all three clip states"
    if c.act_out:
        assert (inp["pred"] == 0).any() and (inp["pred"] > 0).any(), "no clamped row, or only clamped rows"
        assert not inp["dy"][L - 1][inp["pred"] == 0].any()
    if c.loss == "SmoothL1" and B > 1 and not c.weighted:
        assert (inp["td_abs"] < 1).any() and (inp["td_abs"] >= 1).any(), "one side of the SmoothL1 kink"
    if c.special == "tie":
        sel = inp["acts"][2 if c.double else 1][L - 1]
        assert np.array_equal(X.bits(sel[:, 0]), X.bits(sel[:, 1])), "not every row ties"
        assert np.array_equal(X.bits(inp["acts"][0][L - 1][:, 0]), X.bits(inp["acts"][0][L - 1][:, 1]))
        qt = inp["acts"][1][L - 1]
        assert (qt[:, 0] != qt[:, 1]).all() if c.double else (qt[:, 0] == qt[:, 1]).all()
        assert np.array_equal(X.bits(inp["tgt"]), X.bits((inp["reward"] + ((1 - inp["term"]).astype(np.float32) * np.float32(X.GAMMA)) * qt[:, 0]).astype(np.float32)))
    assert any(c2.special == "tie" and c2.double for c2 in X.CASES.values())


@pytest.mark.parametrize("mut", X.MUTANTS)
def test_every_mutant_is_rejected(mut):
    hit = []
    for c, step, env in RUNS:
        if env: continue
        inp = host(c, step)
        if X.failures(X.reference(inp), X.exact(inp), X.restatement(inp, mut)): hit.append("%s-%d" % (c.name, c.batches[step]))
    assert hit, "no case rejects the mutant " + mut
    print(mut, "rejected by", hit)
