"""border_amd.pbt without a GPU: TruncationSelection is deterministic in its seed, never makes a member both source and destination,
never lists a destination twice, respects bounds, ranks NaN last and returns no pairs when frac rounds to zero; run_offline alternates
the group's own calls (a stand-in group records them)."""
import numpy as np
import pytest

from border_amd import pbt

NAMES = ("lr_actor", "gamma")


def population(P, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(P), {"lr_actor": rng.uniform(1e-4, 1e-2, P), "gamma": rng.uniform(0.9, 0.999, P)}


def sched(seed=0, frac=0.25, **kw):
    return pbt.TruncationSelection(frac=frac, factors=(0.8, 1.25), names=NAMES, bounds={"lr_actor": (2e-4, 5e-3), "gamma": (0.0, 0.995)}, seed=seed, **kw)


def test_deterministic_in_its_seed():
    a, b, c = sched(5), sched(5), sched(6)
    same, differs = True, False
    for k in range(6):
        scores, h = population(16, k)
        pa, va = a.step(scores, h)
        pb, vb = b.step(scores, h)
        pc, vc = c.step(scores, h)
        same = same and pa == pb and all(np.array_equal(va[n], vb[n]) for n in NAMES)
        differs = differs or pa != pc or any(not np.array_equal(va[n], vc[n]) for n in NAMES)
    assert same and differs


@pytest.mark.parametrize("P", [2, 3, 4, 8, 9, 64])
@pytest.mark.parametrize("frac", [0.25, 0.5, 0.34])
def test_pairs_are_what_copy_members_accepts(P, frac):
    s = sched(1, frac)
    for k in range(20):
        scores, h = population(P, 100 * P + k)
        pairs, values = s.step(scores, h)
        srcs, dsts = [p[0] for p in pairs], [p[1] for p in pairs]
        n = min(int(frac * P), P // 2)
        assert len(pairs) == n
        assert len(set(dsts)) == len(dsts)                       # no destination twice
        assert not set(srcs) & set(dsts)                         # nobody both source and destination
        assert all(0 <= i < P for i in srcs + dsts)
        order = np.argsort(-scores, kind="stable")
        assert set(dsts) == set(order[P - n:].tolist()) and set(srcs) <= set(order[:n].tolist())
        for name in NAMES:
            lo, hi = s.bounds[name]
            for src, dst in pairs:
                assert lo <= values[name][dst] <= hi
                assert any(values[name][dst] == min(max(h[name][src] * f, lo), hi) for f in s.factors)
            for i in set(range(P)) - set(dsts):
                assert values[name][i] == h[name][i]             # everybody else keeps what came in


def test_nan_ranks_last_and_is_never_a_source():
    scores = np.array([np.nan, 3.0, np.nan, 1.0, 2.0, -np.inf, 0.5, np.nan])
    assert pbt.rank(scores).tolist() == [1, 4, 3, 6, 5, 0, 2, 7]
    h = {"lr_actor": np.full(8, 1e-3), "gamma": np.full(8, 0.95)}
    pairs, _ = sched(0, 0.25).step(scores, h)
    assert sorted(d for _, d in pairs) == [2, 7] and all(s in (1, 4) for s, _ in pairs)
    # more NaN than the bottom holds: the NaN members of the top are no sources; a population of NaN copies nothing
    few = np.array([np.nan, np.nan, 1.0, np.nan])
    pairs, _ = sched(0, 0.5).step(few, {"lr_actor": np.full(4, 1e-3), "gamma": np.full(4, 0.95)})
    assert all(s == 2 for s, _ in pairs) and len(pairs) == 2 and 2 not in [d for _, d in pairs]
    pairs, values = sched(0, 0.5).step(np.full(4, np.nan), {"lr_actor": np.full(4, 1e-3), "gamma": np.full(4, 0.95)})
    assert pairs == [] and values["lr_actor"].tolist() == [1e-3] * 4


def test_frac_rounding_to_zero_returns_no_pairs():
    scores, h = population(3, 0)
    pairs, values = sched(0, 0.25).step(scores, h)   # floor(0.25 * 3) = 0
    assert pairs == [] and all(np.array_equal(values[n], h[n]) for n in NAMES)
    assert sched(0, 0.0).step(*population(16, 1))[0] == []
    with pytest.raises(ValueError):
        sched(0, 0.75)


class FakeGroup:
    """records the calls run_offline makes; a member's score is its lr_actor"""

    def __init__(self, lrs):
        self.h = [{"lr_actor": v, "gamma": 0.9} for v in lrs]
        self.calls = []

    def __len__(self):
        return len(self.h)

    def train_offline(self, buffers, n):
        self.calls.append(("train", n))

    def evaluate(self, evaluators):
        self.calls.append(("eval",))
        return [type("R", (), {"score": m["lr_actor"]})() for m in self.h]

    def get_hyper(self, i, name):
        return self.h[i][name]

    def set_hyper(self, i, name, v):
        self.calls.append(("set", i, name, v))
        self.h[i][name] = v

    def copy_members(self, pairs, hyper=True):
        self.calls.append(("copy", tuple(pairs), hyper))
        for s, d in pairs:
            self.h[d] = dict(self.h[s])


def test_run_offline_alternates_the_groups_calls():
    g = FakeGroup([1e-3, 4e-3, 2e-3, 3e-3])
    seen = []
    hist = pbt.run_offline(g, buffers=None, evaluators=None, total_opts=25, interval=10, schedule=sched(3), on_generation=seen.append)
    assert [e["opt_steps"] for e in hist] == [10, 20, 25] and seen == hist
    kinds = [c[0] for c in g.calls]
    assert kinds == ["train", "eval", "copy", "set", "set", "train", "eval", "copy", "set", "set", "train", "eval"]
    assert [c[1] for c in g.calls if c[0] == "train"] == [10, 10, 5]
    assert hist[0]["pairs"] == [(1, 0)] and g.calls[2] == ("copy", ((1, 0),), True)
    assert hist[0]["scores"] == [1e-3, 4e-3, 2e-3, 3e-3] and hist[0]["hypers"]["lr_actor"] == [1e-3, 4e-3, 2e-3, 3e-3]
    assert hist[0]["set"]["lr_actor"][0] in (4e-3 * 0.8, 5e-3) and hist[1]["hypers"]["lr_actor"][0] == hist[0]["set"]["lr_actor"][0]
    assert hist[-1]["pairs"] == []   # the last generation is evaluated, not selected from
