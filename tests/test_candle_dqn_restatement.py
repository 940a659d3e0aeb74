"""tests/candle_dqn_restatement.py checked against itself and against what is pinned, on the CPU:
  - the committed goldens are what the float32 restatement gives today, bit for bit, and its float32-versus-float64 figures (the
    GPU bars of tests/test_gpu_candle_dqn.py refer to them) are printed (pytest -s) and bounded;
  - update_critic on a batch of two rows worked by hand in float64 - one terminal row and one tie; double and plain targets differ
    on a crafted batch;
  - the SmallRng contract piece by piece: xoshiro256++ against its published outputs, the state of seed 42 from the committed
    seed bytes, gen_range's zone, the WeightedIndex pick at and around a boundary, refused weight lists, the eps schedule."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import candle_dqn_restatement as R  # noqa: E402
import make_golden_candle_dqn as MG  # noqa: E402

F32 = np.float32


@pytest.mark.parametrize("name", sorted(MG.CASES))
def test_goldens_regenerate_bit_for_bit_and_the_float64_figures(golden_dir, name):
    spec, bsz, steps, seed = MG.case(name)
    g = np.load(os.path.join(golden_dir, f"candle_dqn_{name}.npz"))
    q0, t0 = MG.initial(name)
    assert np.array_equal(q0, g["qnet0"]) and np.array_equal(t0, g["qnet_tgt0"])
    ref, ref64 = R.CandleDqnRestatement(spec, q0, t0), R.CandleDqnRestatement(spec, q0, t0, dtype=torch.float64)
    for s in range(steps):
        batch = MG.inputs(name, s)
        for k, v in zip(MG.BATCH_KEYS, batch):
            assert np.array_equal(v, g[f"s{s}_{k}"]), (name, s, k)
        rec = ref.update(*batch)
        ref64.update(*batch)
        for k in MG.PROBE_KEYS + ("grad",):
            assert np.array_equal(ref.probes[k], g[f"s{s}_{k}"]), (name, s, k)
        for k in ("qnet", "qnet_tgt"):
            assert np.array_equal(ref.params(k), g[f"s{s}_{k}"]), (name, s, k)
        for k in R.RECORD_KEYS:
            assert F32(rec[k]) == g[f"s{s}_{k}"], (name, s, k)
        fig = R.f32_f64_figures(ref, ref64)
        print(f"candle_dqn {name} step {s} f32-vs-f64: " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
        for k in R.FIGURE_KEYS:
            assert fig[k] == float(g[f"s{s}_fig_{k}"]), (name, s, k)
            assert fig[k] < 1e-5, (name, s, k, fig[k])   # far inside every GPU bar: no case is ill-conditioned on its own inputs
    # the soft update: interval 2 moves the target after the second opt only
    if spec.soft_update_interval == 2:
        assert np.array_equal(g["s0_qnet_tgt"], g["qnet_tgt0"]) and not np.array_equal(g["s1_qnet_tgt"], g["s0_qnet_tgt"])
        tau, omt = F32(spec.tau), F32(1.0 - spec.tau)
        assert np.array_equal(g["s1_qnet_tgt"], tau * g["s1_qnet"] + omt * g["s0_qnet_tgt"])
        assert np.array_equal(g["s2_qnet_tgt"], g["s1_qnet_tgt"])


def _identity_net(cols):
    """obs 2 -> hidden 2 (identity, inputs kept >= 0) -> A outputs: Q[j] = cols[j] . obs"""
    A = len(cols)
    return np.concatenate([np.eye(2, dtype=np.float32).reshape(-1), np.zeros(2, np.float32), np.asarray(cols, np.float32).reshape(-1), np.zeros(A, np.float32)])


def test_two_rows_by_hand_one_terminal_row_and_one_tie():
    spec = R.CandleDqnSpec(2, 3, (2,), adamw=None, gamma=0.9, double_dqn=False)
    qnet = _identity_net([[1, 0], [0, 1], [1, 1]])              # Q = (x0, x1, x0 + x1)
    tgtn = _identity_net([[2, 0], [0, 2], [0, 2]])              # Q_tgt = (2 x0, 2 x1, 2 x1): columns 1 and 2 tie
    obs = np.array([[1.0, 2.0], [3.0, 0.5]], np.float32)
    nxt = np.array([[0.5, 4.0], [0.25, 1.5]], np.float32)
    act, rew, term = np.array([2, 0]), np.array([1.0, -2.0], np.float32), np.array([1, 0], np.int8)
    ref = R.CandleDqnRestatement(spec, qnet, tgtn)
    rec = ref.update(obs, act, nxt, rew, term, np.array([0, 1], np.int8))
    # float64 by hand: pred = (1 + 2, 3); row 0 terminal -> tgt = 1; row 1: Q_tgt(next) = (0.5, 3, 3): the tie's first index 1, q = 3
    pred = np.array([3.0, 3.0])
    tgt = np.array([1.0, -2.0 + float(F32(0.9)) * 3.0])
    assert ref.probes["y"].tolist()[1] == 1
    assert np.allclose(ref.probes["pred"], pred, rtol=0, atol=1e-6) and np.allclose(ref.probes["tgt"], tgt, rtol=0, atol=1e-6)
    assert abs(rec["loss"] - float(((pred - tgt) ** 2).mean())) < 1e-5
    assert np.allclose(ref.probes["dpred"], 2 * (pred - tgt) / 2, rtol=0, atol=1e-6)
    assert ref.probes["tgt"][0] == rew[0]                       # a terminal row's target IS the reward, bit for bit
    # SmoothL1 on the same rows: |d| = 2 and 2.3: both on the linear side
    spec2 = R.CandleDqnSpec(2, 3, (2,), adamw=None, gamma=0.9, critic_loss="SmoothL1")
    rec2 = R.CandleDqnRestatement(spec2, qnet, tgtn).update(obs, act, nxt, rew, term)
    assert abs(rec2["loss"] - float((np.abs(pred - tgt) - 0.5).mean())) < 1e-5


def test_double_and_plain_targets_differ_on_a_crafted_batch():
    qnet = _identity_net([[1, 0], [0, 1]])                      # online argmax: the larger coordinate
    tgtn = _identity_net([[0, 3], [5, 0]])                      # Q_tgt = (3 x1, 5 x0)
    obs = nxt = np.array([[1.0, 2.0]], np.float32)              # online picks 1 -> Q_tgt[1] = 5; plain max = max(6, 5) = 6
    args = (obs, np.array([0]), nxt, np.zeros(1, np.float32), np.zeros(1, np.int8))
    out = {}
    for dd in (False, True):
        ref = R.CandleDqnRestatement(R.CandleDqnSpec(2, 2, (2,), adamw=None, gamma=1.0, double_dqn=dd), qnet, tgtn)
        ref.update(*args)
        out[dd] = (int(ref.probes["y"][0]), float(ref.probes["q_next"][0]))
    assert out == {False: (0, 6.0), True: (1, 5.0)}


# ------------------------------------------------------------------------------------------------ the SmallRng contract
def test_xoshiro256pp_published_outputs():
    g = R.SmallRng([1, 2, 3, 4])
    assert [g.next_u64() for _ in range(5)] == [41943041, 58720359, 3588806011781223, 3591011842654386, 9228616714210784205]
    g = R.SmallRng([1, 2, 3, 4])
    assert g.next_u32() == 41943041 >> 32


def test_the_state_of_seed_42_comes_from_the_committed_seed_bytes(golden_dir):
    seed = bytes.fromhex(json.load(open(os.path.join(golden_dir, "rng_kat.json")))["seed_from_u64_42"]["seed_hex"])
    assert R.seed_bytes_from_u64(42) == seed
    g = R.SmallRng.from_seed(seed)
    assert g.s == [int.from_bytes(seed[8 * i:8 * i + 8], "little") for i in range(4)] == R.SmallRng.seed_from_u64(42).s
    assert g.s[0] == 0x0a3d32587ba18fa4


def test_gen_f32_takes_the_top_24_bits():
    g, h = R.SmallRng.seed_from_u64(42), R.SmallRng.seed_from_u64(42)
    for _ in range(100):
        v = h.next_u64()
        x = g.gen_f32()
        assert x == F32((v >> 40) * 2.0 ** -24) and 0.0 <= x < 1.0 and x.dtype == np.float32


@pytest.mark.parametrize("A,zone", [(1, (1 << 63) - 1), (2, (1 << 63) - 1), (3, (3 << 62) - 1), (6, (6 << 61) - 1), (18, (18 << 59) - 1),
                                    (1 << 31, (1 << 63) - 1)])
def test_gen_range_zone_and_acceptance(A, zone):
    assert R.range_zone(A) == zone
    g, h = R.SmallRng.seed_from_u64(7), R.SmallRng.seed_from_u64(7)
    for _ in range(200):
        got = g.gen_range(A)
        while True:
            m = h.next_u64() * A
            if (m & R.M64) <= zone:
                break
        assert got == m >> 64 and 0 <= got < A


def test_weighted_index_pick_on_hand_made_weights():
    cum, total = R.cumulative_weights([0.25, 0.25, 0.5])
    assert cum.tolist() == [0.25, 0.5] and total == 1.0
    scale = R.uniform_scale(total)
    assert scale == F32(1.0)   # 1 * (1 - 2^-23) < 1: no step down
    assert R.weighted_pick(cum, F32(0.0) * scale) == 0                              # u = 0
    assert R.weighted_pick(cum, np.nextafter(F32(0.25), F32(0))) == 0               # just under the first boundary
    assert R.weighted_pick(cum, F32(0.25)) == 1                                     # at it: weights <= chosen are counted
    assert R.weighted_pick(cum, np.nextafter(F32(0.5), F32(0))) == 1 and R.weighted_pick(cum, F32(0.5)) == 2
    assert R.weighted_pick(cum, F32(1.0 - 2.0 ** -23)) == 2                         # the largest u
    # a total whose product with 1 - 2^-23 rounds back up to it steps the scale down
    t = F32(3.0)
    s = R.uniform_scale(t)
    assert F32(s * R.MAX_RAND) < t and (s == t or F32(np.nextafter(s, F32(np.inf)) * R.MAX_RAND) >= t)
    # the draw itself: 23 bits of next_u32
    g, h = R.SmallRng.seed_from_u64(42), R.SmallRng.seed_from_u64(42)
    k, cum2, total2, chosen = g.weighted_index([0.25, 0.25, 0.5], detail=True)
    assert chosen == F32(F32(h.next_u32() >> 9) * F32(2.0 ** -23)) and k == R.weighted_pick(cum, chosen)


@pytest.mark.parametrize("w", ([0.0, 0.0, 0.0], [0.5, float("nan"), 0.5], [float("nan"), 1.0], [0.5, -0.25, 1.0]))
def test_zero_total_and_nan_weight_lists_are_refused(w):
    with pytest.raises(ValueError):
        R.SmallRng.seed_from_u64(42).weighted_index(w)


def test_softmax_row_is_f32_and_sums_in_index_order():
    q = np.array([1.0, 3.0, -2.0, 3.0], np.float32)
    p = R.softmax_row(q)
    e = np.exp(q - F32(3.0), dtype=np.float32)
    s = F32(F32(F32(e[0] + e[1]) + e[2]) + e[3])
    assert p.dtype == np.float32 and np.array_equal(p, e / s) and p[1] == p[3]


def test_eps_schedule():
    ex = R.CandleDqnExplorer("eps_greedy", 1.0, 0.02, 1000)
    d = (1.0 - 0.02) / 1000.0
    for n, want in ((0, 1.0), (500, 1.0 - d * 500.0), (1000, max(1.0 - d * 1000.0, 0.02)), (1001, 0.02)):
        ex.n_opts = n
        assert ex.eps() == want, n
    assert abs(R.CandleDqnExplorer("eps_greedy", 1.0, 0.02, 1000, n_opts=1000).eps() - 0.02) < 1e-15


def test_explorer_draw_order_and_counters():
    q = np.array([[0.0, 1.0, 0.5], [2.0, 1.0, 0.0]], np.float32)
    # eps 1: the coin, then one u64 per row in row order
    ex, g = R.CandleDqnExplorer("eps_greedy", 1.0, 1.0, 10, verbose_level=2), R.SmallRng.seed_from_u64(42)
    act = ex.sample(q, True)
    g.gen_f32()
    assert act.tolist() == [g.next_u64() % 3, g.next_u64() % 3] and ex.n_opts == 1 and ex.n_samples_act == 1
    # eps 0: greedy, counted as best at verbosity 2
    ex = R.CandleDqnExplorer("eps_greedy", 0.0, 0.0, 10, verbose_level=2)
    assert ex.sample(q, True).tolist() == [1, 0] and ex.n_samples_best_act == 1
    # eval: one coin per call; the random branch draws ONE action for every row
    ex, g = R.CandleDqnExplorer(), R.SmallRng.seed_from_u64(42)
    for _ in range(500):
        act = ex.sample(q, False)
        if g.gen_f32() < F32(0.01):
            assert act.tolist() == [g.gen_range(3)] * 2
        else:
            assert act.tolist() == [1, 0]
    assert ex.n_samples_act == 0
    # softmax: one WeightedIndex draw per row
    ex, g = R.CandleDqnExplorer("softmax"), R.SmallRng.seed_from_u64(42)
    assert ex.sample(q, True).tolist() == [g.weighted_index(R.softmax_row(r)) for r in q]


def test_small_rng_kat_has_the_keys_of_the_upstream_program_and_is_reproducible():
    """the comparison helper for tools/upstream_kat's `small_rng` section: the keys the Rust program writes, stable values"""
    k = R.small_rng_kat()
    rs = open(os.path.join(HERE, "..", "tools", "upstream_kat", "src", "main.rs")).read()
    for key in k:
        assert f'\\"{key}\\"' in rs, key
    assert k == R.small_rng_kat() and k["seed"] == 42
    g = R.SmallRng.seed_from_u64(42)
    assert k["next_u64"] == [g.next_u64() for _ in range(8)]
    assert [x >> 40 for x in k["next_u64"][:4]] == [int(np.array(b, np.uint32).view(np.float32) * 2.0 ** 24) for b in k["gen_f32_bits"]]
    assert all(0 <= x < 6 for x in k["gen_range_0_6_i64"] + k["gen_u64_mod_6"]) and k["gen_u64_mod_6"] == [x % 6 for x in k["next_u64"][:4]]
    assert all(str(w) in rs for w in R.KAT_WEIGHTS)
