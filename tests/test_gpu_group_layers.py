"""The layer form of a DqnGroup (bdr_agent_group_* over members that do NOT take the one-workgroup step, border_amd/csrc/group_layers.hpp)
against its TWINS: standalone agents with the same configs and seeds, each with a 700-row ring fed the same pushes, stepped one after
the other by `opt`.  Equality is `==` on every element, as in tests/test_gpu_agent_group.py, whose twin scheme this file uses.
Shapes (tests/group_layers_restatement.py SHAPES), the smallest that reach each path of the round:
  (a) in 4, (64, 64), 2 actions, batch 65   one row past fused_ok, ragged third row block, row-block head      8 launches per round
  (b) (a) with double DQN                    three network instances                                             8
  (c) in 6, (64, 192), 5 actions, batch 33   last hidden layer 192 > 128: k_td_dense + k_mean_rows, two dX       11
  (d) in 4, (256, 256), 2 actions, batch 64  the reference's dqn_cartpole                                        11
Every test here fails on a library without the layer form: such a group is refused at build ("does not take the one-workgroup step")."""
import numpy as np
import pytest

from border_amd.trainer import NativeTrainer, TrainerConfig
from tests.group_layers_restatement import SHAPES, fused_ok, head_fused, launches
from tests.test_gpu_agent_group import ARENAS, Ring, assert_same, cfg, run_twins, state, twelve_opts
from tests.test_gpu_group_push import assert_same_ring, draw, group_push, ring_state, row
from tests.test_gpu_group_trainer import CONFIG, ToyEnv, prepare, result, ring_of

pytestmark = pytest.mark.gpu

ENVS = ("BDR_NO_STEP_GATHER", "BDR_NO_MLP_LDS", "BDR_NO_MLP_FUSED", "BDR_NO_MLP_HEAD_FUSE", "BDR_MLP_HEAD_FUSE_WIDE", "BDR_NO_SMALL_GEMM", "BDR_STEP_GRAPH",
        "BDR_GATHER_CHUNKS")
ROUND = {"a": 8, "b": 8, "c": 11, "d": 11}   # launches of one update round, any P


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def clean_env(monkeypatch):
    for k in ENVS: monkeypatch.delenv(k, raising=False)


def shaped(B, name, **kw):
    s = SHAPES[name]
    return cfg(B, s.in_dim, s.units, s.out_dim, s.batch, double_dqn=s.double_dqn, **kw)


def hetero(B, name, n_upd=1):
    """the four members of the issue's list on one shape: (config, ring seed)"""
    first = dict(critic_loss="SmoothL1", tau=0.01, soft_update_interval=2, n_updates_per_opt=n_upd)
    return [
        (shaped(B, name, param_seed=1, **first), 3),
        (shaped(B, name, opt=B.OptimizerConfig.AdamW(1e-3, wd=0.05), critic_loss="Mse", tau=1.0, soft_update_interval=1, n_updates_per_opt=n_upd, param_seed=2), 4),
        (shaped(B, name, discount_factor=0.9, clip_td_err=(-0.5, 0.5), soft_update_interval=3, n_updates_per_opt=n_upd, param_seed=3), 5),
        (shaped(B, name, param_seed=11, **first), 13),
    ]


def seeds_only(B, name, P, **kw):
    return [(shaped(B, name, param_seed=100 + i, tau=0.1, **kw), 200 + i) for i in range(P)]


def run_group(B, members, schedule, expect=None):
    """tests/test_gpu_agent_group.py run_group, with the form checked through bdr_agent_group_info"""
    g = B.DqnGroup.build([c for c, _ in members])
    assert g.form == "layers" and g.info()["n_members"] == len(members)
    if expect is not None: assert g.launches_per_round == expect
    rings = [Ring(B, c, seed) for c, seed in members]
    bufs = [r.rb for r in rings]
    losses = [[] for _ in members]
    def step(record, only=None):
        if only is not None:
            m = g.members[only]
            if record: losses[only].append(m.opt_with_record(bufs[only])["loss"])
            else: m.opt(bufs[only])
        elif record:
            for l, rec in zip(losses, g.opt_with_record(bufs)): l.append(rec["loss"])
        else:
            g.opt(bufs)
    def push(n):
        for r in rings: r.push(n)
    schedule(step, push)
    g.sync()
    out = [state(m, r, l) for m, r, l in zip(g.members, rings, losses)]
    g.close()
    for r in rings: r.rb.close()
    return out


def four_opts(step, push):
    for k in range(4):
        step(k % 4 == 0)
        push(50)


def test_the_shapes_reach_the_paths_they_are_meant_to():
    """the twins' own path, from the restatement of fused_ok / update_critic: none of (a)-(d) takes the one-workgroup step, (a) and (b)
    take the row-block head, (c) and (d) k_td_dense + k_mean_rows; C1 (batch 64) does take the one-workgroup step"""
    assert [fused_ok(SHAPES[k]) for k in "abcd"] == [False] * 4 and fused_ok(SHAPES["c1"])
    assert [head_fused(SHAPES[k]) for k in "abcd"] == [True, True, False, False]
    assert {k: len(launches(SHAPES[k])) for k in "abcd"} == ROUND


@pytest.mark.parametrize("n_upd", [1, 2])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_heterogeneous_members_equal_their_twins(B, name, n_upd, monkeypatch):
    """Adam / SmoothL1 / tau 0.01 / interval 2; AdamW wd 0.05 / Mse / hard update; gamma 0.9 with clip_td_err / interval 3; a second seed
    of the first - twelve group opts with pushes in between (the rings wrap) and a Record on every fourth"""
    clean_env(monkeypatch)
    members = hetero(B, name, n_upd)
    want = run_twins(B, members, twelve_opts)
    got = run_group(B, members, twelve_opts, expect=ROUND[name])
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")
        assert len(g["losses"]) == 3 and g["n_opts"] == 12
    assert not (got[0]["arenas"]["qnet"] == got[3]["arenas"]["qnet"]).all()
    assert not (got[0]["arenas"]["qnet_tgt"] == got[0]["arenas"]["qnet"]).all() and (got[1]["arenas"]["qnet_tgt"] == got[1]["arenas"]["qnet"]).all()   # tau 0.01 / tau 1


@pytest.mark.parametrize("n_upd", [1, 2])
def test_the_reference_shape_equals_its_twins(B, n_upd, monkeypatch):
    """(d) Mlp[256, 256], batch 64: three members, four opts"""
    clean_env(monkeypatch)
    members = hetero(B, "d", n_upd)[:3]
    want = run_twins(B, members, four_opts)
    got = run_group(B, members, four_opts, expect=11)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")
        assert len(g["losses"]) == 1 and g["n_opts"] == 4


def test_four_launch_tail_when_the_head_is_switched_off(B, monkeypatch):
    """BDR_NO_MLP_HEAD_FUSE=1 on shape (a): members and group take k_td_dense + k_mean_rows + one more layer and dX (11 launches), same bits as the
    twins stepped with the row-block head"""
    clean_env(monkeypatch)
    members = hetero(B, "a")
    want = run_twins(B, members, twelve_opts)
    monkeypatch.setenv("BDR_NO_MLP_HEAD_FUSE", "1")
    got = run_group(B, members, twelve_opts, expect=11)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")


def test_member_calls_mix_with_group_calls(B, monkeypatch):
    """group opt, member 2 alone through bdr_agent_opt (its own layer path, on the group's stream), group opt - against the twins"""
    clean_env(monkeypatch)
    def sched(step, push):
        step(False); push(20)
        step(False, only=2); step(True, only=2)
        push(20); step(True)
    members = hetero(B, "a")
    want = run_twins(B, members, sched)
    got = run_group(B, members, sched)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")
    assert [g["n_opts"] for g in got] == [2, 2, 4, 2]


def test_steps_and_pushes_without_a_synchronise(B, monkeypatch):
    """fifty group opts back to back (the step ring of 8 slots is rewritten six times while launches are queued), then 40 x (grouped
    push of one row, group opt) with no synchronise either, against twins fed by rb.push"""
    clean_env(monkeypatch)
    assert 50 >= 6 * B.DqnGroup.STAGING_DEPTH
    members = hetero(B, "a")[:3]
    cols = [draw(np.random.default_rng(90 + i), 4, 2, 40) for i in range(3)]
    want_mid, want, want_rings = [], [], []
    for i, (c, seed) in enumerate(members):
        a, ring = B.Dqn.build(c), Ring(B, c, seed)
        for _ in range(50): a.opt(ring.rb)
        a.sync()
        want_mid.append({k: a.get_params(k) for k in ARENAS})
        for k in range(40):
            ring.rb.push(*row(cols[i], k)); a.opt(ring.rb)
        a.sync()
        want_rings.append(ring_state(ring.rb))
        want.append(state(a, ring, []))
        a.close(); ring.rb.close()
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [Ring(B, c, seed) for c, seed in members]
    bufs = [r.rb for r in rings]
    for _ in range(50): g.opt(bufs)
    g.sync()
    for i, m in enumerate(g.members):
        for k in ARENAS: assert (m.get_params(k) == want_mid[i][k]).all(), (i, k)
    for k in range(40):
        group_push(g, cols, k, bufs); g.opt()
    g.sync()
    for i, (m, r) in enumerate(zip(g.members, rings)):
        assert_same_ring(ring_state(r.rb), want_rings[i], f"member {i}")
        assert_same(state(m, r, []), want[i], f"member {i}")
        assert m.n_opts == 90
    g.close()
    for r in rings: r.rb.close()


def test_the_launch_count_does_not_depend_on_the_number_of_members(B, monkeypatch):
    """shape (a): 8 launches per round for 2 and for 9 members, 3 * 8 launches after three opts.  Shape (d), the reference's
    dqn_cartpole: 11 = the 10 launches update_critic enqueues (pack, three layers, TD rows, loss mean, two input gradients, the
    grouped weight gradient, reduce + Adam) + the gather."""
    clean_env(monkeypatch)
    counts = []
    for P in (2, 9):
        members = seeds_only(B, "a", P)
        g = B.DqnGroup.build([c for c, _ in members])
        rings = [Ring(B, c, s) for c, s in members]
        assert g.form == "layers" and g.launches_per_round == 8 and g.kernel_launches == 0
        for _ in range(3): g.opt([r.rb for r in rings])
        g.sync()
        counts.append(g.kernel_launches)
        g.close()
        for r in rings: r.rb.close()
    assert counts == [24, 24]
    g = B.DqnGroup.build([shaped(B, "d", param_seed=5)])
    assert g.form == "layers" and g.launches_per_round == 11
    g.close()
    g = B.DqnGroup.build([cfg(B, param_seed=5)])   # Mlp[64, 64] at batch 32: today's group, one launch
    assert g.form == "one_workgroup" and g.launches_per_round == 1
    g.close()


def test_twenty_four_members(B, monkeypatch):
    clean_env(monkeypatch)
    members = seeds_only(B, "a", 24)
    def two(step, push):
        step(False); step(False)
    want = run_twins(B, members, two)
    got = run_group(B, members, two, expect=8)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")
        assert g["n_opts"] == 2


@pytest.mark.parametrize("mode", ["eps_greedy", "eval"])
@pytest.mark.parametrize("name", ["c", "d"])
def test_acting_equals_the_twins(B, name, mode, monkeypatch):
    """20 group.sample calls with opts in between on nets 192 and 256 wide: actions, every bdr_sample_info field (so the explorer
    streams), the action values; then a subset call that leaves the other members untouched"""
    clean_env(monkeypatch)
    members = hetero(B, name)[:3]
    in_dim = SHAPES[name].in_dim
    def prepare_one(i, a):
        if mode == "eval": a.eval()
        else: a.train()
        a.set_explorer(B.EpsilonGreedy(final_step=10), seed=70 + i)
    rows = np.random.default_rng(8).standard_normal((22, 3, in_dim)).astype(np.float32)
    want_act, want_info, want_q, want_last = [], [], [], []
    for i, (c, seed) in enumerate(members):
        a, ring = B.Dqn.build(c), Ring(B, c, seed)
        prepare_one(i, a)
        acts, infos, qs = [], [], []
        for k in range(20):
            act, info = a.sample(rows[k, i][None], return_info=True)
            acts.append(int(act[0])); infos.append(info)
            if k % 10 == 3: qs.append(a.qvalues(rows[k, i][None])[0])
            if k % 5 == 4: a.opt(ring.rb)
        if i != 1: acts.append(int(a.sample(rows[20, i][None])[0]))   # the subset call: members 0 and 2
        want_last.append(a.sample(rows[21, i][None], return_info=True))
        want_act.append(acts); want_info.append(infos); want_q.append(qs)
        a.close(); ring.rb.close()
    g = B.DqnGroup.build([c for c, _ in members])
    assert g.form == "layers"
    rings = [Ring(B, c, seed) for c, seed in members]
    for i, m in enumerate(g.members): prepare_one(i, m)
    for k in range(20):
        act, info = g.sample(rows[k], return_info=True)
        for i in range(3):
            assert int(act[i]) == want_act[i][k], (k, i)
            assert info[i] == want_info[i][k], (k, i)
        if k % 10 == 3:
            for i, q in enumerate(g.qvalues(rows[k])):
                w = want_q[i][k // 10]
                assert q.shape == w.shape and (q == w).all(), (k, i)
        if k % 5 == 4: g.opt([r.rb for r in rings])
    act = g.sample(rows[20], members=[0, 2])
    assert int(act[0]) == want_act[0][20] and int(act[2]) == want_act[2][20]
    act, info = g.sample(rows[21], return_info=True)   # member 1's explorer stream and counters did not move in the subset call
    for i in range(3):
        assert int(act[i]) == int(want_last[i][0][0]) and info[i] == want_last[i][1], i
    g.close()
    for r in rings: r.rb.close()


def test_group_loop_equals_two_single_loops(B, monkeypatch):
    """DqnGroup.train on two members of shape (a), toy environments of 5-9-step episodes, against two Trainer.train runs on twins"""
    clean_env(monkeypatch)
    members = hetero(B, "a")[:2]
    want = []
    for i, (c, seed) in enumerate(members):
        a, rb = B.Dqn.build(c), ring_of(B, c, seed)
        prepare(B, i, a)
        ev = []
        st = NativeTrainer(TrainerConfig(**CONFIG)).train(ToyEnv(4, 300 + i), a, rb, (4,), np.float32, on_event=lambda e, o, name, sc: ev.append((e, o, name, sc)))
        want.append(result(a, rb, ev, st))
        a.close(); rb.close()
    g = B.DqnGroup.build([c for c, _ in members])
    assert g.form == "layers"
    for i, m in enumerate(g.members): prepare(B, i, m)
    bufs = [ring_of(B, c, seed) for c, seed in members]
    events = [[] for _ in members]
    stats = g.train([ToyEnv(4, 300 + i) for i in range(2)], bufs, TrainerConfig(**CONFIG), on_event=lambda m, e, o, name, sc: events[m].append((e, o, name, sc)))
    g.sync()
    got = [result(m, rb, events[i], stats[i]) for i, (m, rb) in enumerate(zip(g.members, bufs))]
    for i, (gt, w) in enumerate(zip(got, want)):
        for k in ARENAS: assert (gt["arenas"][k] == w["arenas"][k]).all(), (i, k)
        assert gt["len"] == w["len"] and gt["head"] == w["head"], i
        for a, b in zip(gt["rows"], w["rows"]): assert (a.view(np.uint8) == b.view(np.uint8)).all(), i
        assert (gt["ixs"] == w["ixs"]).all(), i
        assert gt["stats"] == w["stats"], (i, gt["stats"], w["stats"])
        assert gt["events"] == w["events"], i
        assert gt["n_opts"] == w["n_opts"] == 30
    g.close()
    for rb in bufs: rb.close()


def test_refusals_leave_nothing_behind(B, monkeypatch):
    clean_env(monkeypatch)
    ok = hetero(B, "a")[:2]
    def refused(configs, *words):
        with pytest.raises(B.BdrError) as e:
            B.DqnGroup.build(configs)
        for w in words: assert w in str(e.value), str(e.value)
    # create
    refused([ok[0][0], cfg(B, param_seed=9)], "member 1", "one-workgroup")                         # a layer-path member 0, a one-workgroup member 1
    refused([cfg(B, param_seed=9), ok[0][0]], "member 1", "one-workgroup")                         # and the other way round: the existing wording
    refused([ok[0][0], shaped(B, "c")], "member 1", "shape")
    refused([ok[0][0], shaped(B, "a", critic_loss="Mse"), cfg(B, 4, (64, 64), 2, 66)], "member 2", "shape")   # batch size is part of the shape
    refused([cfg(B, 4, (320, 64), 2, 64)], "member 0", "wider than 256")
    refused([cfg(B, 4, (64, 64, 64, 64), 2, 65)], "member 0", "4 layers")                          # five layers
    refused([ok[0][0], shaped(B, "a", opt=B.OptimizerConfig.AdamW(1e-3, amsgrad=True))], "member 1", "amsgrad")
    refused([ok[0][0], shaped(B, "a", n_updates_per_opt=2)], "member 1", "n_updates_per_opt")
    monkeypatch.setenv("BDR_NO_SMALL_GEMM", "1")
    refused([ok[0][0]], "member 0", "BDR_NO_SMALL_GEMM")
    monkeypatch.delenv("BDR_NO_SMALL_GEMM")
    # opt / push / set_prioritized
    def sched(step, push):
        step(False); step(True)
    want = run_twins(B, ok, sched)
    g = B.DqnGroup.build([c for c, _ in ok])
    rings = [Ring(B, c, seed) for c, seed in ok]
    bufs = [r.rb for r in rings]
    g.opt(bufs)
    with pytest.raises(B.BdrError) as e:
        g.set_prioritized(True)
    assert "prioritized" in str(e.value) and not g.prioritized
    per = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4, per_config=B.PerConfig()), (4,), np.float32)
    cols = draw(np.random.default_rng(0), 4, 2, 80)
    per.push(*cols)
    empty = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4), (4,), np.float32)
    for wrong, word in ((per, "prioritized"), (empty, "empty")):
        with pytest.raises(B.BdrError) as e:
            g.opt([bufs[0], wrong])
        assert "member 1" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(B.BdrError) as e:
        group_push(g, [cols, cols], 0, [bufs[0], per])
    assert "member 1" in str(e.value) and "prioritized" in str(e.value), str(e.value)
    with pytest.raises(B.BdrError):
        g.opt([bufs[0], bufs[0]])       # one ring for two members
    assert g.kernel_launches == 8      # the one accepted opt
    losses = [rec["loss"] for rec in g.opt_with_record(bufs)]
    for i, (m, ring) in enumerate(zip(g.members, rings)):
        assert_same(state(m, ring, [losses[i]]), want[i], f"member {i}")   # heads, sizes, index streams and adam_step were untouched
    g.close()
    per.close(); empty.close()
    for ring in rings: ring.rb.close()
