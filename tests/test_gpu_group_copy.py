"""copy_members of BcGroup, IqlGroup, AwacGroup and CandleSacGroup (csrc/group_copy.hpp through the C ABI): training state copied
between members in one launch.  Everything is compared bit for bit (np.array_equal) over every (model, role) the parameter views serve
(tests/group_copy_cases.py has the kinds' configs, shapes and state).

A group has P = 4 members over views of one dataset (a ring of capacity 128 holding 100 rows):
  member 0, member 1   one seed (initial parameters, noise stream) and one view seed (index stream); member 1's learning rates are 1.5 x
                       member 0's and nothing else differs
  member 2, member 3   differ from member 0 and from each other in the seed, the view seed and every hyperparameter; of a candle SAC group
                       members 0 - 2 tune their entropy coefficient (Auto) and member 3 has a fixed one
The prologue every scenario starts with: three rounds in train mode, then one update_on_batch of member 3's own - its n_opts and, where
an update draws noise, its noise counter then differ from every other member's - and member 3 goes to eval mode."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_copy_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS, VIEW_SEEDS = (3, 3, 5, 6), (50, 50, 52, 53)
ROUNDS = 3
BASE = [(k, "partial_block") for k in K.SHAPES]   # one small shape per kind for the scenarios that are not about the shape


def lib():
    import border_amd
    return border_amd


@pytest.fixture(scope="module")
def B():
    border_amd = lib()
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def member_hypers(kind, shape):
    h0 = K.hypers(kind, 0, shape[1])
    h1 = {n: v * 1.5 if n.startswith("lr") else v for n, v in h0.items()}
    return [h0, h1, K.hypers(kind, 2, shape[1]), K.hypers(kind, 3, shape[1], auto=False)]


class Run:
    """a group of four over views of one dataset, after the prologue"""

    def __init__(self, B, kind, name, prologue=True):
        self.kind, self.shape = kind, K.SHAPES[kind][name]
        self.hs = member_hypers(kind, self.shape)
        self.g = getattr(B, K.GROUPS[kind]).build([K.config(B, kind, self.shape, self.hs[i], SEEDS[i]) for i in range(4)])
        self.owner = K.dataset(B, self.shape)
        self.views = [self.owner.view(s) for s in VIEW_SEEDS]
        if prologue:
            for _ in range(ROUNDS):
                self.g.opt(self.views)
            self.g.members[3].update_on_batch(*K.own_batch(kind, self.shape, 3))
            self.g.members[3].eval()

    def states(self):
        return [K.state(self.kind, m) for m in self.g.members]

    def own(self, i):
        """what a copy leaves the destination's: n_opts, the mode, and eight draws at its noise counter (BC has no noise stream)"""
        m = self.g.members[i]
        return {"n_opts": m.n_opts, "train": m.is_train(), "noise": m.draw_noise(8) if self.kind != "bc" else np.zeros(0)}

    def close(self):
        self.g.sync()
        self.g.close()
        for v in self.views:
            v.close()
        self.owner.close()


@functools.lru_cache(maxsize=None)
def control(kind, name):
    """the same group without a copy: member 2's state after the prologue and three more rounds, and what is members 1's and 3's own"""
    r = Run(lib(), kind, name)
    for _ in range(ROUNDS):
        r.g.opt()
    out = {"state2": r.states()[2], 1: r.own(1), 3: r.own(3)}
    r.close()
    return out


@pytest.mark.parametrize("kind,name", K.CASES)
def test_a_clone_continues_as_its_source(B, kind, name):
    r = Run(B, kind, name)
    g = r.g
    s = r.states()
    assert not K.same(s[0], s[1]) and not K.same(s[0], s[3])
    launches, per_round = g.kernel_launches, g.launches_per_round
    g.copy_members([(0, 1), (0, 3)], hyper=True)
    assert g.kernel_launches == launches + 1 and g.launches_per_round == per_round
    s = r.states()
    K.assert_same(s[1], s[0], "member 1 right after the copy")
    K.assert_same(s[3], s[0], "member 3 right after the copy")
    for i in (1, 3):
        for n in r.hs[i]:   # (member 3 of a candle SAC group has no ent_coef_lr and no target_entropy to take)
            assert g.get_hyper(i, n) == r.hs[0][n], (i, n)
    for k in range(ROUNDS):
        g.opt()
        s = r.states()
        K.assert_same(s[1], s[0], f"member 1, round {k + 1} after the copy")
    assert not K.same(s[3], s[0])   # its own seed, mode and index stream
    want = control(kind, name)
    K.assert_same(s[2], want["state2"], "member 2 against the group that never copied")
    for i in (1, 3):
        own = r.own(i)
        assert own["n_opts"] == want[i]["n_opts"] and own["train"] == want[i]["train"] and np.array_equal(own["noise"], want[i]["noise"]), (i, own, want[i])
    assert g.members[3].n_opts == g.members[0].n_opts + 1 and (not K.HAS_MODE[kind] or (g.members[0].is_train() and not g.members[3].is_train()))
    r.close()


@pytest.mark.parametrize("kind,name", BASE)
def test_a_state_only_copy_and_set_hyper_of_every_source_value_equal_a_copy_with_hyper(B, kind, name):
    a, b = Run(B, kind, name), Run(B, kind, name)
    a.g.copy_members([(0, 1), (0, 3)], hyper=True)
    b.g.copy_members([(0, 1), (0, 3)], hyper=False)
    for i in (1, 3):
        for n in b.hs[i]:
            assert b.g.get_hyper(i, n) == b.hs[i][n], (i, n)   # a state-only copy leaves them the destination's
            b.g.set_hyper(i, n, b.g.get_hyper(0, n))
    for k in range(ROUNDS):
        a.g.opt(); b.g.opt()
        for i, (x, y) in enumerate(zip(a.states(), b.states())):
            K.assert_same(y, x, (i, k))
    a.close(); b.close()


COPIES = ([(0, 1)], [(2, 3)], [(1, 2), (0, 3)], [(3, 0)], [(2, 1), (2, 0)])


@pytest.mark.parametrize("kind,name", BASE)
def test_slots_are_rewritten(B, kind, name):
    """twelve copies, more than the eight slots of the pinned segment ring, interleaved with rounds and never synchronised, against
    the same calls with a sync after each"""
    out = []
    for sync in (False, True):
        r = Run(B, kind, name)
        assert r.g.COPY_STAGING_DEPTH == 8
        for k in range(12):
            r.g.copy_members(COPIES[k % len(COPIES)], hyper=k % 3 != 0)
            if sync: r.g.sync()
            if k % 2 == 0:
                r.g.opt()
                if sync: r.g.sync()
        out.append(r.states())
        r.close()
    for i, (x, y) in enumerate(zip(*out)):
        K.assert_same(x, y, i)


@pytest.mark.parametrize("kind,name", BASE)
def test_one_launch_whatever_the_number_of_pairs(B, kind, name):
    r = Run(B, kind, name)
    g = r.g
    per_round = g.launches_per_round
    n0 = g.kernel_launches
    g.copy_members([(0, 1)])
    assert g.kernel_launches == n0 + 1
    g.copy_members([(0, 1), (2, 3)])   # P / 2 pairs
    assert g.kernel_launches == n0 + 2
    g.copy_members([])                 # nothing to do, nothing launched
    assert g.kernel_launches == n0 + 2
    g.opt()
    assert g.kernel_launches == n0 + 2 + per_round and g.launches_per_round == per_round
    r.close()


@pytest.mark.parametrize("kind,name", BASE + [("bc", "partial_block_mfma")])
def test_derived_copies_follow(B, kind, name):
    """acting after a copy: the group's sample of the destination, and the destination's own sample on both act paths, return the
    source's bits (every member in eval mode) - also where they had acted, and so staged what acting derives, before the copy"""
    r = Run(B, kind, name)
    g = r.g
    for m in g.members:
        m.eval()
    rows = np.random.default_rng(11).standard_normal((5, r.shape[0])).astype(np.float32)

    def own(i, path):
        g.members[i].set_act_path(path)
        return g.members[i].sample_raw(rows)
    before = g.sample(rows)
    assert not np.array_equal(before[1], before[0]) and not np.array_equal(before[3], before[0])
    for path in ("layers", "fused"):
        assert not np.array_equal(own(1, path), own(0, path))
    g.copy_members([(0, 1), (0, 3)])
    after = g.sample(rows)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
    for i in (1, 3):
        assert np.array_equal(after[i], after[0]), i
        for path in ("layers", "fused"):
            assert np.array_equal(own(i, path), own(0, path)), (i, path)
            assert np.array_equal(own(i, path), after[0]), (i, path)
    r.close()


@pytest.mark.parametrize("kind,name", BASE)
def test_refusals_name_the_pair_and_move_nothing(B, kind, name):
    r, c = Run(B, kind, name), Run(B, kind, name)
    g = r.g
    before, launches = r.states(), g.kernel_launches
    n_arenas = {"bc": 4, "awac": 14, "iql": 18, "candle_sac": 15}[kind]
    too_many = 65535 // n_arenas + 1
    refused = [
        ([(0, 4)], r"pair 0 \(0 -> 4\)"), ([(0, 1), (4, 2)], r"pair 1 \(4 -> 2\)"),            # an index >= P
        ([(2, 3), (1, 1)], r"pair 1 \(1 -> 1\)"),                                             # src == dst
        ([(0, 1), (2, 1)], r"pair 1 \(2 -> 1\).*destination of an earlier pair"),             # a destination listed twice
        ([(0, 1), (1, 2)], r"pair 1 \(1 -> 2\).*destination of another pair"),                # a destination that is also a source
        ([(1, 2), (0, 1)], r"pair 1 \(0 -> 1\).*source of another pair"),
        ([(0, 1)] * too_many, rf"{too_many} pairs of {n_arenas} arenas.*65535"),               # more segments than grid y holds
    ]
    for pairs, msg in refused:
        for hyper in (True, False):
            with pytest.raises(B.BdrError, match=msg) as e:
                g.copy_members(pairs, hyper=hyper)
            assert e.value.code == 1   # BDR_ERR_INVALID
    assert g.kernel_launches == launches
    for i, (x, y) in enumerate(zip(r.states(), before)):
        K.assert_same(x, y, i)
    for i in range(4):
        assert g.members[i].n_opts == c.g.members[i].n_opts
        for n in r.hs[i]:
            assert g.get_hyper(i, n) == r.hs[i][n]
    # the step counters and the staging slots too: a round continues as in the group that was never asked
    g.opt(); c.g.opt()
    for i, (x, y) in enumerate(zip(r.states(), c.states())):
        K.assert_same(x, y, i)
    r.close(); c.close()
