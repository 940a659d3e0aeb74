"""Host self-test of tests/dqn_forward_reference.py (no GPU): the sequential f32 restatement of every forward layer passes the three
criteria on CPU-evaluated inputs of the small cases and reproduces RESTATEMENT_RATIO (so LAMBDA cannot drift from what sets it), and
every mistake a forward kernel could make - restatement(mutate=...) - fails them on at least one case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dqn_forward_reference as Fw  # noqa: E402

# (B, A, n_stack) of the cases the mutations run on: the staged-image conv1 shape with one image, and the smallest k (n_stack 1) with three
SMALL = {c[0]: c[:3] for c in Fw.RESTATEMENT_CASES}


@pytest.fixture(scope="module")
def inputs():
    """B -> (inputs of the online instance on obs with the target set as `params_other`, shapes); computed once, never written to."""
    out = {}
    for Bsz, (_, A, ns) in SMALL.items():
        q, tg, shapes = Fw.case_params(A, ns, Bsz)
        obs = Fw.case_batch(Bsz, A, ns)[0]
        out[Bsz] = Fw.cpu_inputs(Fw.unflat(q, shapes), obs, params_other=Fw.unflat(tg, shapes))
    return out


def test_restatement_passes_and_reproduces_the_recorded_ratios():
    worst = Fw.restatement_ratios()       # both instances, both arithmetics of conv2 / conv3, every RESTATEMENT_CASE
    assert {k: round(v, 3) for k, v in worst.items()} == Fw.RESTATEMENT_RATIO, worst
    assert Fw.LAMBDA == {k: max(1.0, 4.0 * v) for k, v in Fw.RESTATEMENT_RATIO.items()}
    assert all(c in Fw.CASES for c in Fw.RESTATEMENT_CASES) and len(Fw.RESTATEMENT_CASES) == 3


@pytest.mark.parametrize("split", [False, True], ids=["exact", "split"])
def test_restatement_passes_every_criterion(inputs, split):
    for Bsz, inp in inputs.items():
        val = Fw.restatement(inp, split)
        v = Fw.check_all(Fw.reference(inp, split), val, Fw.LAMBDA)
        assert set(v) == set(Fw.OPS) and all(x.elements == val[k].size for k, x in v.items())
        for k in ("a1", "a2", "a3", "h1"):
            assert (val[k] == 0).any() and (val[k] > 0).any(), (Bsz, k)


def test_edge_images_are_in_the_batches_and_zero_images_give_the_bias(inputs):
    """The B = 7 batch holds an all-zero and an all-255 image; on the zero image every product is 0 and a1 is relu(b1) to the bit."""
    inp = inputs[7]
    (z0, _), (f0, _) = Fw.EDGE_ROWS[7]
    assert (inp["obs"][z0] == 0).all() and (inp["obs"][f0] == 255).all()
    mask, val = Fw.bias_only(inp)
    assert mask[z0].all() and not mask[f0].any()
    a1 = Fw.restatement(inp, only=("a1",))["a1"]
    assert np.array_equal(a1[mask].view(np.uint32), np.ascontiguousarray(val[mask]).view(np.uint32))
    ops = Fw.reference(inp, only=("a1",))
    assert (ops["a1"].extra[z0] == 0).all() and (ops["a1"].extra[f0] > 0).any()


MUTATIONS = [
    # (output, mistake, split, B of the case)
    ("a1", dict(swap_khkw=True), False, 3), ("a2", dict(swap_khkw=True), True, 1), ("a3", dict(swap_khkw=True), True, 1),
    ("a1", dict(drop_tap=(7, 7)), False, 1), ("a2", dict(drop_tap=(0, 3)), True, 1), ("a3", dict(drop_tap=(2, 0)), False, 3),
    ("a1", dict(drop_last_kstep=True), False, 7), ("a2", dict(drop_last_kstep=True), True, 3), ("a3", dict(drop_last_kstep=True), True, 1),
    ("a1", dict(bias_xor=True), False, 3), ("a2", dict(bias_xor=True), True, 1), ("a3", dict(bias_xor=True), False, 1),
    ("h1", dict(bias_xor=True), False, 1), ("q", dict(bias_xor=True), False, 3),
    ("a1", dict(no_scale=True), False, 1),
    ("a1", dict(row_shift=True), False, 3), ("a2", dict(row_shift=True), True, 3), ("a3", dict(row_shift=True), True, 7),
    # five of the six products: one of the two of relative size 2^-8 is missing.  (The three smallest kept products are <= 2^-16 |x| |w|
    # each, of either sign: without (2, 0) the restatement's a2 ratio on the B = 1 case only moves from 0.24 to 0.49, inside lambda.
    # A per-element bound of sqrt(n) u S cannot see those; the fused kernel's bit identity with the two-launch form is what pins them.)
    ("a2", dict(kept=tuple(t for t in Fw.KEPT if t != (1, 0))), True, 1), ("a3", dict(kept=tuple(t for t in Fw.KEPT if t != (0, 1))), True, 3),
    ("h1", dict(drop_kslice=7), False, 1), ("h1", dict(drop_kslice=0), False, 3),
    ("a2", dict(other_w=True), True, 1), ("a2", dict(other_w=True), False, 7),
]


@pytest.mark.parametrize("name,mistake,split,Bsz", MUTATIONS, ids=["%s-%s%s-B%d" % (n, next(iter(m)), "-split" if s else "", b) for n, m, s, b in MUTATIONS])
def test_every_mistake_fails(inputs, name, mistake, split, Bsz):
    inp = inputs[Bsz]
    ops = Fw.reference(inp, split, only=(name,))
    good = Fw.restatement(inp, split, only=(name,))
    Fw.check_all(ops, good, Fw.LAMBDA)
    bad = Fw.restatement(inp, split, only=(name,), mutate={name: mistake})
    with pytest.raises(AssertionError, match=r"\[%s\]" % name):
        Fw.check_all(ops, bad, Fw.LAMBDA)
    # a row shift touches one position per image and nothing else
    if "row_shift" in mistake:
        diff = (bad[name] != good[name]).reshape(Bsz, -1, bad[name].shape[-1])
        assert diff[:, -1].any() and not diff[:, :-1].any()


def test_split_terms_are_exact_and_nearest():
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * np.float32(3.7)
    t0, t1, t2 = Fw.split3_rn(x)
    assert np.array_equal(t0.astype(np.float64) + t1.astype(np.float64) + t2.astype(np.float64), x.astype(np.float64))
    for t in (t0, t1, t2):
        assert not (t.view(np.uint32) & np.uint32(0xffff)).any()
    nz = x != 0
    assert (np.abs(x - t0)[nz] <= np.abs(x[nz]) * 2.0 ** -8).all()
