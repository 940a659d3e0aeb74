"""Host self-test of tests/dqn_backward_reference.py: the checker of the DQN backward kernels accepts a correct kernel and rejects
a wrong one.  No GPU: the "kernel" is the sequential float32 restatement on a CPU evaluation of a B = 3 batch, and the wrong kernels
are that restatement with one row dropped from a dW sum, one tap dropped from a dX, kh / kw swapped in one dX weight row, the ReLU
mask not applied, one chunk's partial added twice, or conv1's 1/255 left out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_backward_reference as R  # noqa: E402

B, A, NS = 3, 6, 4


@pytest.fixture(scope="module")
def world():
    p0, shapes = R.case_params(A, NS, 31)
    obs, act, nobs, rew, term = R.case_batch(B, A, NS, 32)
    inp = R.cpu_inputs(p0, shapes, obs, act, td=(nobs, rew, term))
    return inp, R.reference(inp), R.restatement(inp)


def test_reduction_lengths_and_tap_classes():
    assert [R.taps_c3(i) for i in range(9)] == [1, 2, 3, 3, 3, 3, 3, 2, 1]
    assert [R.taps_c2(i) for i in range(20)] == [1, 1] + [2] * 16 + [1, 1]
    assert sorted({R.taps_c3(i) * R.taps_c3(j) for i in range(9) for j in range(9)}) == [1, 2, 3, 4, 6, 9]
    assert sum(R.taps_c3(i) * R.taps_c3(j) for i in range(9) for j in range(9)) == 441      # tap-tiles per image of DxC3Pos
    assert sorted({R.taps_c2(i) * R.taps_c2(j) for i in range(20) for j in range(20)}) == [1, 2, 4]


def test_the_restatement_passes_every_criterion(world):
    inp, ops, rest = world
    assert set(rest) == set(R.OPS) == set(R.LAMBDA)
    v = R.check_all(ops, rest, R.LAMBDA)
    # the case is not vacuous: masked units and an action without rows exist, and so do unmasked ones
    for k in ("dh1", "dy3", "dy2", "dy1", "gW5", "gb5"):
        assert (ops[k].S == 0).any() and (ops[k].S > 0).any(), k
    assert all(x.worst_ratio <= 1 and x.sharp_ratio <= R.LAMBDA[x.name] for x in v.values())
    assert all(lam >= 1 for lam in R.LAMBDA.values())


def test_the_f64_reference_is_autograd(world):
    """reference() against torch autograd in f64 through the whole network, started from the same dq (masks agree: same activations)."""
    import torch
    inp, ops, _ = world
    p = [torch.from_numpy(x).double().requires_grad_(True) for x in inp["params"]]
    x = torch.from_numpy(inp["obs"]).double() / 255
    F = torch.nn.functional
    a1 = F.conv2d(x, p[0], p[1], stride=4).relu(); a2 = F.conv2d(a1, p[2], p[3], stride=2).relu(); a3 = F.conv2d(a2, p[4], p[5]).relu()
    h1 = F.linear(a3.flatten(1), p[6], p[7]).relu()
    q = F.linear(h1, p[8], p[9]).gather(1, torch.from_numpy(inp["act"])[:, None])[:, 0]
    (q * torch.from_numpy(inp["dq"]).double()).sum().backward()
    for k, i in R.GRAD_INDEX.items():
        g = p[i].grad.numpy()
        # the chain's intermediates are the f32 restatement's (rounded), and a unit within rounding of 0 may flip in f64: loose
        assert np.abs(g - ops[k].ref).max() <= 1e-4 * np.abs(g).max() + 1e-12, k


MUTATIONS = [
    # one row dropped from a dW sum
    ("gW5", dict(skip=0)), ("gW4", dict(skip=1)), ("gW3", dict(skip=70)), ("gW2", dict(skip=200)), ("gW1", dict(skip=1199)),
    # one tap (one term of l1's 512) dropped from a dX
    ("dy3", dict(drop_term=100)), ("dy2", dict(drop_tap=(1, 1))), ("dy2", dict(drop_tap=(0, 0))), ("dy1", dict(drop_tap=(2, 3))),
    # kh and kw swapped in one dX weight row
    ("dy2", dict(swap="live")), ("dy1", dict(swap="live")),   # (the input channel with the most unmasked units: a dead channel shows nothing)
    # the ReLU mask not applied
    ("dh1", dict(relu=False)), ("dy3", dict(relu=False)), ("dy2", dict(relu=False)), ("dy1", dict(relu=False)),
    # one chunk's partial (a 32-row tile; one image for conv1) added twice
    ("gW3", dict(twice=(32, 64))), ("gW2", dict(twice=(224, 243))), ("gW1", dict(twice=(400, 800))), ("gW4", dict(twice=(2, 3))),
    # conv1's 1/255 left out
    ("gW1", dict(scale=False)),
]


@pytest.mark.parametrize("name,mut", MUTATIONS, ids=["%s-%s" % (n, "-".join("%s=%s" % kv for kv in m.items()).replace(" ", "")) for n, m in MUTATIONS])
def test_a_wrong_kernel_is_rejected(world, name, mut):
    inp, ops, rest = world
    if mut.get("swap") == "live":
        mut = dict(swap=int(np.argmax((inp["a2" if name == "dy2" else "a1"] > 0).sum((0, 1, 2)))))
    bad = R.restatement(inp, only=(name,), mutate={name: mut})[name]
    assert not np.array_equal(bad, rest[name])
    v = R.check(ops[name], bad, R.LAMBDA[name])
    assert not v.ok, (name, mut, v)
    assert R.KERNEL[name] in v.message and name in v.message
    if mut.get("relu") is False:
        assert v.n_nonzero_where_zero > 0 and "(a)" in v.message      # an unmasked unit is caught as a nonzero where S == 0
    if name in ("dy2", "dy1"):
        assert "tap class" in v.message and "position (" in v.message
    with pytest.raises(AssertionError, match=name):
        R.check_all(ops, {name: bad}, R.LAMBDA)


def test_one_dropped_row_is_far_above_the_sharp_bound(world):
    """How loud a single lost row is: it moves more than 20 % of conv3 dW's elements above 4 sqrt(n) u S (the share measured at 3185
    rows when the check was designed; here the sum has 147 rows), while the end-to-end tolerance (2e-4 of the variable's largest entry)
    would need it to carry 2e-4 of the whole sum.  The share cannot come near 100 %: a row touches only the elements whose a2 entry
    and dy3 entry are both nonzero in it, and both are ReLU-sparse."""
    inp, ops, rest = world
    bad = R.restatement(inp, only=("gW3",), mutate={"gW3": dict(skip=70)})["gW3"]
    v = R.check(ops["gW3"], bad, 4.0)
    assert v.n_over_sharp > 0.20 * v.elements, v


# the rows of `python tests/dqn_backward_reference.py` that are cheap enough for a test, and the entries of the table that they set
SMALL_CASES = [c for c in R.CASES if c[0] <= 7]
SET_BY_SMALL_CASES = ("gW4", "gb4", "dy3", "gW3", "gb3", "gW2", "gb2", "gW1", "gb1")


@pytest.fixture(scope="module")
def small_case_ratios():
    out = []
    for (Bsz, A_, ns, _) in SMALL_CASES:
        p0, shapes = R.case_params(A_, ns, 100 + Bsz)
        obs, act, nobs, rew, term = R.case_batch(Bsz, A_, ns, 200 + Bsz)
        inp = R.cpu_inputs(p0, shapes, obs, act, td=(nobs, rew, term))
        out.append(R.sharp_ratios(R.reference(inp), R.restatement(inp)))
    return out


def test_lambda_is_four_times_the_measured_restatement_ratio(small_case_ratios):
    """RESTATEMENT_RATIO is a copied record: the B = 1, 3 and 7 cases recomputed here stay within it (to its three decimals) and
    reproduce the nine entries that they set, and LAMBDA is 4 x the table floored at 1 - nothing else."""
    assert [c[0] for c in SMALL_CASES] == [1, 3, 7]
    half_digit = 5e-4
    for r in small_case_ratios:
        for k in R.OPS:
            assert r[k] <= R.RESTATEMENT_RATIO[k] + half_digit, (k, r[k])
    for k in SET_BY_SMALL_CASES:
        assert abs(max(r[k] for r in small_case_ratios) - R.RESTATEMENT_RATIO[k]) <= half_digit, k
    assert R.LAMBDA == {k: max(1.0, 4.0 * R.RESTATEMENT_RATIO[k]) for k in R.OPS}
