"""Host self-test of tests/iqn_layer_reference.py (no GPU): the f64 reference is autograd, the sequential f32 restatement passes every
criterion and sets the recorded lambda, every listed wrong kernel is rejected, and every case of tests/test_gpu_iqn_layers.py is
non-vacuous."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iqn_layer_reference as Q  # noqa: E402

SMALL = [n for n, c in Q.CASES.items() if c.small]
GRADS = lambda ops: [k for k in ops if k.startswith("g")]


@pytest.fixture(scope="module")
def worlds():
    """name -> (inp, ops, restatement) of the small cases, and of n33-chunked (the ragged dW of the mutants)."""
    out = {}
    for name in SMALL + ["n33-chunked"]:
        c = Q.CASES[name]
        p, pt = Q.case_params(c)
        inp = Q.cpu_inputs(c.spec, p, pt, Q.case_batch(c))
        out[name] = (inp, Q.reference(inp), Q.restatement(inp))
    return out


def test_small_cases_are_the_ones_the_table_names():
    assert SMALL == ["tiny-padded", "n33-follow-up", "cnn-b3"]


def _autograd64(c, p_flat, pt_flat, batch):
    """Iqn::update_critic in float64 autograd for either feature extractor: the flat gradient in reference order."""
    s = c.spec
    obs, act, nobs, rew, term, tau_p, tau_t = batch
    d = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    unflat = lambda flat: [d(a) for a in _unflatten(flat, s.shapes())]
    n_psi = len(s.shapes3()[0])

    def fwd(p, x, tau):
        if s.cnn:
            h = d(np.asarray(x).reshape(len(x), -1, 84, 84)) / 255
            h = F.conv2d(h, p[0], p[1], stride=4).relu(); h = F.conv2d(h, p[2], p[3], stride=2).relu()
            psi = F.conv2d(h, p[4], p[5], stride=1).relu().flatten(1)
        else:
            psi = d(x)
            for j in range(0, n_psi, 2):
                psi = F.linear(psi, p[j], p[j + 1])
                if j < n_psi - 2 or s.act_out: psi = psi.relu()
        Bn, N = tau.shape
        ci, _ = Q.cos_args(tau, s.E)                                           # the device's f32 constants fl(pi (i + 1)), products exact
        cos = torch.cos(d(tau).reshape(-1, 1) * d(ci)[None, :])
        x = psi.unsqueeze(1) * F.linear(cos, p[n_psi], p[n_psi + 1]).relu().reshape(Bn, N, s.F)
        f = p[n_psi + 2:]
        for j in range(0, len(f), 2):
            x = F.linear(x, f[j], f[j + 1])
            if j < len(f) - 2: x = x.relu()
        return x
    p = [t.requires_grad_(True) for t in unflat(p_flat)]
    with torch.no_grad():
        zt = fwd(unflat(pt_flat), nobs, tau_t)
        a2 = zt.mean(1).argmax(-1)
        k = d((np.float32(1) - np.asarray(term, np.float32)) * np.float32(s.gamma))
        tgt = d(rew)[:, None] + k[:, None] * zt[torch.arange(c.B), :, a2]      # [B][Nt]
    pred = fwd(p, obs, tau_p)[torch.arange(c.B), :, torch.as_tensor(act)]      # [B][Np]
    diff = tgt[:, :, None] - pred[:, None, :]
    w = (d(tau_p)[:, None, :] - (diff < 0).double()).abs()
    (w * F.smooth_l1_loss(diff, torch.zeros_like(diff), reduction="none", beta=1.0)).mean().backward()
    return np.concatenate([t.grad.numpy().ravel() for t in p])


def _unflatten(flat, shapes):
    out, o = [], 0
    for sh in shapes:
        n = int(np.prod(sh)); out.append(np.asarray(flat[o:o + n]).reshape(sh)); o += n
    return out


@pytest.mark.parametrize("name", ["n33-follow-up", "cnn-b3"])
def test_the_f64_reference_is_autograd(worlds, name):
    """Every weight / bias gradient of reference() - evaluated layer by layer on float32 intermediates - against float64 autograd through
    the whole update (local, either feature extractor; for the Mlp case also edge_inputs.IqnRef).  The intermediates carry float32
    roundings through at most seven layers, each ~sqrt(n) u ~ 1e-6 of its scale: 2e-5 of a variable's largest entry; a layout, mask,
    permutation or scale mistake is O(1)."""
    c = Q.CASES[name]
    inp, ops, _ = worlds[name]
    p, pt = Q.case_params(c)
    batch = Q.case_batch(c)
    flats = [_autograd64(c, p, pt, batch)]
    if not c.spec.cnn:
        import edge_inputs as EI
        s = c.spec
        spec = EI.IqnSpec(in_dim=s.in_dim, psi_units=tuple(s.psi_units), feature_dim=s.F, embed_dim=s.E, f_units=tuple(s.m_units), n_actions=s.A, gamma=s.gamma)
        flats.append(EI.IqnRef(spec, p, pt).update(*batch)["grad"])
    for flat in flats:
        want = Q.device_grads(flat.astype(np.float64), c.spec)      # (internal_params rounds to f32: fine at 2e-5)
        assert set(want) == set(GRADS(ops))
        for k, g in want.items():
            assert np.abs(ops[k].ref - g).max() <= 2e-5 * np.abs(g).max(), (k, np.abs(ops[k].ref - g).max() / np.abs(g).max())
            assert np.abs(g).max() > 0


@pytest.mark.parametrize("name", SMALL + ["n33-chunked"])
def test_the_restatement_passes_every_criterion(worlds, name):
    inp, ops, rest = worlds[name]
    assert set(rest) == set(ops)
    v = Q.check_all(ops, rest, Q.LAMBDA)
    print("restatement ratios %s: " % name + " ".join("%s %.3f" % (k, x.sharp_ratio) for k, x in v.items()))


def test_lambda_is_four_times_the_recorded_restatement_ratio(worlds):
    """RESTATEMENT_RATIO is a copied record of `python tests/iqn_layer_reference.py`: the small cases recomputed here stay within it (to
    its three decimals) and reproduce RESTATEMENT_SMALL, their own largest; lambda is 4 x the table floored at 1 - nothing else."""
    half_digit = 5e-4
    worst = {}
    for name in SMALL:
        _, ops, rest = worlds[name]
        for k, r in Q.sharp_ratios(ops, rest).items():
            k = Q._family(k)
            assert k in Q.RESTATEMENT_RATIO and r <= Q.RESTATEMENT_RATIO[k] + half_digit, (name, k, r)
            worst[k] = max(worst.get(k, 0.0), r)
    assert set(worst) == set(Q.RESTATEMENT_SMALL)
    for k, r in worst.items():
        assert abs(r - Q.RESTATEMENT_SMALL[k]) <= half_digit, (k, r)
    for k in ("gWf1", "dlin", "gWf7", "dy2", "cos"):
        assert Q.LAMBDA[k] == max(1.0, 4.0 * Q.RESTATEMENT_RATIO[Q._family(k)])


def _rejected(ops, inp, name, mut, label):
    val = Q.restatement(inp, only=(name,), mutate={name: mut})[name]
    v = Q.check(ops[name], val, Q.LAMBDA[name])
    print("mutant %-60s %s: (a) %d  (b) %d  (c) %d elements, largest sharp ratio %.3g against lambda %.3g"
          % (label, name, v.n_nonzero_where_zero, v.n_over_worst, v.n_over_sharp, v.sharp_ratio, Q.LAMBDA[name]))
    assert not v.ok
    return v


def test_wrong_dw_kernels_are_rejected(worlds):
    """n33-chunked: M = 2145 rows = 67 tiles of 32 + one row, 8 chunks of 9 tiles."""
    inp, ops, _ = worlds["n33-chunked"]
    M = 65 * 33
    assert M == 67 * 32 + 1 and Q.dw_chunks(M) == 8 and math.ceil(68 / 8) == 9
    for name in ("gWf1", "gWc"):
        assert _rejected(ops, inp, name, dict(drop_rows=(9 * 32 * 3 + 64, 9 * 32 * 3 + 96)), "one 32-row tile dropped from the fourth dW chunk").n_over_sharp > 0
        assert _rejected(ops, inp, name, dict(drop_rows=(M - 1, M)), "the last one-row tile dropped").n_over_sharp > 0
    assert _rejected(ops, inp, "gWf1", dict(had_shift=7), "Hadamard group index off by one, first row of sample 7 (dW)").n_over_sharp > 0
    assert _rejected(ops, inp, "hf1", dict(had_shift=7), "Hadamard group index off by one, first row of sample 7 (forward)").n_over_sharp > 0


def test_wrong_merge_backward_and_padding_are_rejected(worlds):
    """The masks and the padding are criterion (a)'s: the reference has S == 0 there, so ANY nonzero is rejected, however small."""
    inp, ops, _ = worlds["n33-chunked"]
    assert _rejected(ops, inp, "dpsi", dict(mask=False), "dpsi without the psi > 0 mask").n_nonzero_where_zero > 0
    assert _rejected(ops, inp, "dlin", dict(mask=False), "dlin without the phi > 0 mask").n_nonzero_where_zero > 0
    inp, ops, _ = worlds["tiny-padded"]
    assert _rejected(ops, inp, "phi", dict(pad_nonzero=3), "one padding column of phi nonzero (1e-30)").n_nonzero_where_zero == 1


def test_wrong_target_kernels_are_rejected(worlds):
    inp, ops, _ = worlds["tiny-padded"]
    assert inp["z_tgt"].shape[1] == 100
    a_mean, _ = Q.target_choice(inp["z_tgt"]); a_last, _ = Q.target_choice(inp["z_tgt"], last_point=True)
    assert (a_mean != a_last).any()
    assert _rejected(ops, inp, "tgt", dict(last_point=True), "tgt with the argmax of the last percent point").n_over_sharp > 0
    assert _rejected(ops, inp, "tgt", dict(tail_unwritten=True), "tgt's Nt tail beyond 64 left unwritten").n_over_sharp > 0


@pytest.mark.parametrize("name", list(Q.CASES))
def test_cases_are_not_vacuous(name):
    """phi, every hidden activation and (behind a ReLU) psi have zero and positive entries; every row of dz has its one nonzero; every
    action but EMPTY_ACTION has a row (as far as the rows go: tiny-padded has 3 for 64 actions); a terminated and a live row; and the
    target's argmax cannot depend on the summation order."""
    c = Q.CASES[name]
    s = c.spec
    p, pt = Q.case_params(c)
    inp = Q.cpu_inputs(s, p, pt, Q.case_batch(c), restate_chain=False)
    both = lambda x: bool((x == 0).any() and (x > 0).any())
    assert both(inp["phi"][:, :s.F]) and all(both(h[:, :u]) for h, u in zip(inp["f_act"], s.m_units))
    assert (inp["psi"] > 0).any() and (not s.mask_psi or both(inp["psi"][:, :s.F]))
    if not s.mask_psi:
        assert (inp["psi"][:, :s.F] < 0).any()
    assert ((inp["f_dy"][-1] != 0).sum(1) == 1).all()
    act = inp["act"]
    assert Q.EMPTY_ACTION not in act
    assert set(act.tolist()) == set(range(1, s.A)) if c.B >= s.A - 1 else len(set(act.tolist())) == c.B
    assert inp["term"][0] == 1 and inp["term"][1] == 0
    ok, gap = Q.tgt_gap_ok(inp["z_tgt"])
    assert ok and gap > 3, gap
    assert Q.uses_b3(c) == name.startswith("split")


def test_split_constant_and_path_conditions():
    """SPLIT_C against a brute-force split of random floats (the bound holds, and is within 4 x of the worst found), and the kernels each
    case is meant to select."""
    rng = np.random.default_rng(0)

    def bf16(x):   # round to nearest even on the upper 16 bits
        b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
        return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)

    def split(x):
        t0 = bf16(x); r1 = (x - t0).astype(np.float32); t1 = bf16(r1); t2 = (r1 - t1).astype(np.float32)
        assert (bf16(t2) == t2).all() and (t0.astype(np.float64) + t1 + t2 == x).all()
        return t0.astype(np.float64), t1.astype(np.float64), t2.astype(np.float64)
    x, y = (rng.standard_normal(1 << 20).astype(np.float32) for _ in range(2))
    (x0, x1, x2), (y0, y1, y2) = split(x), split(y)
    dropped = np.abs(x1 * y2 + x2 * y1 + x2 * y2) / np.abs(x.astype(np.float64) * y)
    assert Q.SPLIT_C / 4 < dropped.max() <= Q.SPLIT_C, dropped.max() / Q.SPLIT_C
    C = Q.CASES
    assert Q.split_outputs(C["split-fused"]) == ("hf1", "dlin", "dpsi", "phi", "gWf1", "gbf1") == Q.split_outputs(C["split-n32"])
    assert Q.split_outputs(C["split-ragged"]) == ("hf1", "dlin", "dpsi") and Q.split_outputs(C["exact"]) == ()
    assert [Q.dw_chunks(C[n].B * C[n].Np) for n in ("tiny-padded", "n33-chunked", "n33-follow-up", "n10-chunked", "split-fused", "split-ragged")] == [1, 8, 1, 8, 8, 8]
