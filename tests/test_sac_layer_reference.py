"""Host self-test of tests/sac_layer_reference.py (no GPU): the f64 reference equals f64 autograd of a plain torch SAC step, the
sequential-f32 restatement passes every criterion and reproduces the recorded ratio table, every case reaches the branches it is
there for, and every wrong kernel (MUTANTS) is rejected."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sac_layer_reference as X  # noqa: E402

HOST_CASES = [c for c in X.CASES.values()]


@pytest.fixture(scope="module")
def host():
    """inp, reference and restatement of every case, computed once."""
    out = {}
    for c in HOST_CASES:
        inp = X.host_inputs(c)
        out[c.name] = (inp, X.reference(inp), X.restatement(inp))
    return out


# ------------------------------------------------------------------------------------------------ reference == autograd
def _torch_step(c, inp):
    """A plain SAC step in f64 torch on the same numbers (unpadded), autograd for every gradient."""
    fl = inp["_flat"]
    obs, act, nobs, rew, term, z1, z2 = (torch.from_numpy(np.asarray(x, np.float64)) for x in fl["batch"])
    B, A = obs.shape[0], c.A

    def net(flat, name):
        ps, o = [], 0
        for s in X.shapes(c, name):
            n = int(np.prod(s)); ps.append(torch.from_numpy(np.asarray(flat[o:o + n], np.float64).reshape(s)).requires_grad_(True)); o += n
        return ps
    pi, pi1 = net(fl["pi"], "pi"), net(fl["pi1"], "pi")
    qs, qts = [net(x, "q") for x in fl["q"]], [net(x, "q") for x in fl["qt"]]
    nt, L = len(c.pi), len(c.q) + 1
    keep = {}

    def actor(P, x, z, tag):
        h = x
        for l in range(nt):
            pre = h @ P[2 * l].t() + P[2 * l + 1]; keep["%s.pre%d" % (tag, l)] = pre
            if pre.requires_grad: pre.retain_grad()
            h = pre.relu(); keep["%s.h%d" % (tag, l)] = h
        mean = h @ P[2 * nt].t() + P[2 * nt + 1]; e = h @ P[2 * nt + 2].t() + P[2 * nt + 3]
        if mean.requires_grad: mean.retain_grad(); e.retain_grad()
        s = e.exp(); sd = s.clamp(X.f32(c.lo), X.f32(c.hi)).exp()
        a = (sd * z + mean).tanh()
        logp = (-X.LN_SQRT_2PI - 0.5 * z * z).sum(1) - ((1 - a * a) + X.f32(c.eps)).log().sum(1)
        keep.update({tag + ".mean": mean, tag + ".e": e, tag + ".s": s, tag + ".sd": sd, tag + ".a": a, tag + ".logp": logp})
        return a, logp

    def critic(P, x, tag):
        h = x
        for l in range(L):
            pre = h @ P[2 * l].t() + P[2 * l + 1]
            keep["%s.pre%d" % (tag, l)] = pre
            if pre.requires_grad: pre.retain_grad()
            h = pre.relu() if l < L - 1 else pre
            keep["%s.h%d" % (tag, l)] = h
        return h[:, 0]
    a, logp = actor(pi, obs, z1, "pi")
    xs = [torch.cat([obs, a], 1) for _ in range(c.NC)]           # one input tensor per critic: its gradient is that critic's dxq
    for x in xs: x.retain_grad()
    keep["xq_a"] = xs
    qa = torch.stack([critic(qs[i], xs[i], "q%d.a" % i) for i in range(c.NC)])
    alpha = math.exp(float(np.asarray(inp["actor"]["log_alpha"], np.float64)[0]))
    # torch.min over critics takes the FIRST minimum on a tie, as the kernel does
    qmin = qa.min(0).values
    keep["qmin"] = qmin
    loss_actor = (alpha * logp - qmin).mean()
    loss_actor.backward()
    with torch.no_grad():
        a2, logp2 = actor([p.detach() for p in pi1], nobs, z2, "pi'")
        qt = torch.stack([critic([p.detach() for p in qts[i]], torch.cat([nobs, a2], 1), "q%d.t" % i) for i in range(c.NC)])
        tgt = X.f32(c.reward_scale) * rew + (1 - term) * X.f32(c.gamma) * (qt.min(0).values - alpha * logp2)
    keep["tgt"] = tgt
    loss_c = 0
    for i in range(c.NC):
        for p in qs[i]: p.grad = None
        q = critic(qs[i], torch.cat([obs, act], 1), "q%d.c" % i)
        d = q - tgt
        rows = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5) if c.loss == "SmoothL1" else d * d
        keep["loss_rows%d" % i] = rows
        li = rows.mean()
        li.backward()
        loss_c = loss_c + li.item() / c.NC
    return keep, pi, qs, loss_actor.item(), loss_c


@pytest.mark.parametrize("name", list(X.CASES))
def test_reference_equals_f64_autograd(name):
    c = X.CASES[name]
    inp = X.host_inputs(c, dtype=np.float64)
    ops = X.reference(inp)
    keep, pi, qs, loss_actor, loss_c = _torch_step(c, inp)
    Lp, Lq = X.layers(c, "pi"), X.layers(c, "q")
    nt, L, A = len(c.pi), len(Lq), c.A
    seen = []

    def same(opname, want, cols=None):
        got = ops[opname].ref
        want = want.detach().numpy() if hasattr(want, "detach") else np.asarray(want)
        if got.ndim == 2: got = got[:, :want.shape[1]] if cols is None else got[:, cols]
        scale = max(np.abs(want).max(), 1e-30)
        assert np.abs(got.reshape(want.shape) - want).max() <= 1e-9 * scale, (opname, np.abs(got.reshape(want.shape) - want).max(), scale)
        seen.append(opname)
    for tag in ("pi", "pi'"):
        for l in range(nt): same("%s.h%d" % (tag, l), keep["%s.h%d" % (tag, l)])
        for k in ("mean", "e", "a", "logp"): same("%s.%s" % (tag, k), keep["%s.%s" % (tag, k)])
    same("pi.s", keep["pi.s"]); same("pi.sd", keep["pi.sd"])
    same("pi.gmean", keep["pi.mean"].grad); same("pi.ge", keep["pi.e"].grad)
    for l in range(nt): same("pi.dy%d" % l, keep["pi.pre%d" % l].grad)
    same("tgt", keep["tgt"])
    for i in range(c.NC):
        for t in "act":
            for l in range(L): same("q%d.%s.h%d" % (i, t, l), keep["q%d.%s.h%d" % (i, t, l)])
        for l in range(L):   # (the last layer: the selection one-hot and the TD dout, column 0 of the padded output)
            same("q%d.a.dy%d" % (i, l), -c.B * keep["q%d.a.pre%d" % (i, l)].grad)   # the step carries d qmin / d h; the loss's -1 / B comes in ga
            same("q%d.c.dy%d" % (i, l), keep["q%d.c.pre%d" % (i, l)].grad)
        if not c.fused: same("q%d.a.dxq" % i, -c.B * keep["xq_a"][i].grad)
    # weight gradients: the chunk partials added up, and the reduce's sum, against autograd; weight [out][in] <-> [Kp][Np]
    for net, P, lay in [("pi", pi, Lp)] + [("q%d" % i, qs[i], Lq) for i in range(c.NC)]:
        for l, (i_, o_, kp, np_, _) in enumerate(lay):
            parts = sorted(k for k in ops if k.startswith("%s.dW%d.part" % (net, l)))
            for got in (sum(ops[k].ref for k in parts), ops["%s.dW%d.sum" % (net, l)].ref):
                gw, gb = got[:kp * np_].reshape(kp, np_), got[kp * np_:]
                for g, w in ((gw[:i_, :o_].T, P[2 * l].grad.numpy()), (gb[:o_], P[2 * l + 1].grad.numpy())):
                    assert np.abs(g - w).max() <= 1e-9 * max(np.abs(w).max(), 1e-30), (net, l)
                assert not gw[i_:].any() and not gw[:, o_:].any() and not gb[o_:].any()
            seen.extend(parts + ["%s.dW%d.sum" % (net, l)])
    if c.fused:   # the block partials: 32 rows each, of log p + target, log p, qmin and every critic's loss rows
        tgt_e = X.f32(c.ent[1]) if c.ent[0] == "Auto" else 0.0
        rows = [keep["pi.logp"] + tgt_e, keep["pi.logp"], keep["qmin"]] + [keep["loss_rows%d" % i] for i in range(c.NC)]
        nb = (c.B + 31) // 32
        want = np.zeros((len(rows), nb * 32)); want[:, :c.B] = np.stack([r.detach().numpy() for r in rows])
        same("lrow", want.reshape(len(rows), nb, 32).sum(2))
    assert abs(ops["loss_actor"].ref[0] - loss_actor) <= 1e-9 * abs(loss_actor)
    assert abs(ops["loss_critic"].ref[0] - loss_c) <= 1e-9 * abs(loss_c)
    assert set(ops) - set(seen) == {"loss_actor", "loss_critic"}, set(ops) - set(seen)   # (compared just above)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_passes_every_criterion_and_reproduces_the_table(host):
    worst = {}
    for name, (inp, ops, rest) in host.items():
        assert set(ops) == set(X.device(inp)) == set(rest), name
        bad = X.failures(ops, rest)
        assert not bad, (name, bad[:3])
        assert not X.exact_checks(inp), name
        for k, v in X.kind_ratios(ops, rest).items(): worst[k] = max(worst.get(k, 0.0), v)
    # the recorded table, output by output (critics and chunks folded), to its three decimals; lambda is 4 x it floored at 1, and 1 for
    # the row-wise outputs - nothing else
    assert set(worst) == set(X.RESTATEMENT_RATIO), set(worst) ^ set(X.RESTATEMENT_RATIO)
    for k, v in X.RESTATEMENT_RATIO.items():
        assert abs(worst[k] - v) < 5.5e-4, (k, worst[k], v)
        assert X.LAMBDA[k] == (1.0 if X.family(k) == "row" else max(1.0, 4.0 * v)), k
    assert set(X.LAMBDA) == set(X.RESTATEMENT_RATIO)


def test_host_simulation_in_f32_passes_too(host):
    """simulate()'s own float32 values (numpy's summation order) are a second 'device': they pass as well."""
    for name, (inp, ops, _) in host.items():
        bad = X.failures(ops, X.device(inp))
        assert not bad, (name, bad[:3])


# ------------------------------------------------------------------------------------------------ non-vacuity
def test_every_case_reaches_its_branches(host):
    for name, (inp, _, _) in host.items():
        assert not X.branch_checks(inp), (name, X.branch_checks(inp))
    c = X.CASES["chunked-dw"]                      # the later batches of the sequence on one agent
    for step, Bn in enumerate(c.batches):
        if step: assert not X.branch_checks(X.host_inputs(c, B=Bn, step=step)), (c.name, Bn)


# ------------------------------------------------------------------------------------------------ mutants
MUTANT_CASE = {"drop_dw_row": "a17-edge", "drop_reduce_chunk": "chunked-dw", "alias_last_block": "a32", "shift_action_columns": "a17-edge",
               "tie_to_higher": "saturated", "ignore_inr": "saturated", "drop_eps": "a17-edge", "target_from_old_actor": "a17-edge",
               "padding_nonzero": "tiny-padded"}
MUTANT_HITS = {"drop_dw_row": "q0.dW0.part", "drop_reduce_chunk": "q0.dW0.sum", "alias_last_block": "pi.h0", "shift_action_columns": "pi.gmean",
               "tie_to_higher": ".a.dy", "ignore_inr": "pi.ge", "drop_eps": "pi.logp", "target_from_old_actor": "pi'.", "padding_nonzero": "pi.mean"}


@pytest.mark.parametrize("mut", X.MUTANTS)
def test_every_mutant_is_rejected(host, mut):
    assert set(MUTANT_CASE) == set(X.MUTANTS)
    inp, ops, _ = host[MUTANT_CASE[mut]]
    v = X.verdicts(ops, X.restatement(inp, mut))
    bad = [k for k, x in v.items() if not x.ok]
    assert bad and all(MUTANT_HITS[mut] in k for k in bad), (mut, bad)
