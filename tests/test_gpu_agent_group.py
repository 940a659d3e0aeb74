"""A group of small Mlp DQN agents stepped in one launch (bdr_agent_group_*, border_amd.DqnGroup) against its TWINS: standalone
agents with the same configs and seeds, each with a ring fed the same pushes, stepped one after the other by `opt` / `sample`.
Equality is `==` on every element: parameters, target parameters, gradient and moment arenas, losses, n_opts, the rings' index
streams, action sequences and every bdr_sample_info field."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARENAS = ("qnet", "qnet_tgt", "grad", "exp_avg", "exp_avg_sq")
ENVS = ("BDR_NO_STEP_GATHER", "BDR_NO_MLP_LDS", "BDR_NO_MLP_FUSED")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def cfg(B, in_dim=4, units=(64, 64), A=2, bs=32, opt=None, **kw):
    return B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.MlpConfig(in_dim=in_dim, units=tuple(units), out_dim=A),
                                                    opt_config=opt or B.OptimizerConfig.Adam(1e-3)),
                       batch_size=bs, device=0, **kw)


def hetero(B, n_upd):
    """the five members of the issue's table: (config, ring seed)"""
    a = dict(in_dim=4, units=(64, 64), A=2, bs=32, double_dqn=True, critic_loss="SmoothL1", tau=0.01, soft_update_interval=2)
    return [
        (cfg(B, n_updates_per_opt=n_upd, param_seed=1, **a), 3),
        (cfg(B, 4, (64, 64), 2, 64, critic_loss="Mse", tau=1.0, soft_update_interval=1, n_updates_per_opt=n_upd, param_seed=2), 4),   # 8 blocks per phase
        (cfg(B, 3, (32,), 3, 17, opt=B.OptimizerConfig.AdamW(2e-3, wd=0.05), soft_update_interval=3, tau=0.05, n_updates_per_opt=n_upd, param_seed=3), 5),
        (cfg(B, 6, (64, 32, 64), 5, 32, discount_factor=0.9, clip_td_err=(-0.5, 0.5), n_updates_per_opt=n_upd, param_seed=4), 6),
        (cfg(B, n_updates_per_opt=n_upd, param_seed=11, **a), 13),
    ]


class Ring:
    """a 700-capacity ring and the generator of its pushes (same seed -> same rows for a member and its twin)"""
    def __init__(self, B, c, seed, capacity=700, first=300):
        q = c.model_config.q_config
        self.in_dim, self.A = q.in_dim, q.out_dim
        self.rng = np.random.default_rng(1000 + seed)
        self.rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=capacity, seed=seed), (self.in_dim,), np.float32)
        self.push(first)

    def push(self, n):
        r = self.rng
        self.rb.push(r.standard_normal((n, self.in_dim)).astype(np.float32), r.integers(0, self.A, (n, 1)).astype(np.int64),
                     r.standard_normal((n, self.in_dim)).astype(np.float32), r.standard_normal(n).astype(np.float32),
                     (r.random(n) < .1).astype(np.int8), np.zeros(n, np.int8))


def state(agent, ring, losses):
    agent.sync()
    return {"arenas": {k: agent.get_params(k) for k in ARENAS}, "ixs": ring.rb.sample_indices(40), "losses": losses, "n_opts": agent.n_opts}


def assert_same(got, want, what=""):
    for k in ARENAS:
        assert (got["arenas"][k] == want["arenas"][k]).all(), (what, k)
    assert np.isfinite(got["arenas"]["qnet"]).all(), what
    assert (got["ixs"] == want["ixs"]).all(), (what, "index stream")
    assert got["losses"] == want["losses"], (what, "losses")
    assert got["n_opts"] == want["n_opts"], (what, "n_opts")


def run_twins(B, members, schedule):
    """every member's twin, one at a time: schedule(step_fn(record: bool) -> loss or None, ring, member index)"""
    out = []
    for i, (c, seed) in enumerate(members):
        a, ring = B.Dqn.build(c), Ring(B, c, seed)
        losses = []
        def step(record, a=a, ring=ring, losses=losses):
            if record: losses.append(a.opt_with_record(ring.rb)["loss"])
            else: a.opt(ring.rb)
        schedule(lambda record, only=None: step(record) if only in (None, i) else None, lambda n: ring.push(n))
        out.append(state(a, ring, losses))
        a.close(); ring.rb.close()
    return out


def run_group(B, members, schedule):
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [Ring(B, c, seed) for c, seed in members]
    bufs = [r.rb for r in rings]
    losses = [[] for _ in members]
    def step(record, only=None):
        if only is not None:   # one member alone, through its own Agent::opt
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


def twelve_opts(step, push):
    for k in range(12):
        step(k % 4 == 0)
        push(50)   # the ring wraps (capacity 700)


_twins = {}


def twins_of_test1(B, n_upd):
    if n_upd not in _twins:
        _twins[n_upd] = run_twins(B, hetero(B, n_upd), twelve_opts)
    return _twins[n_upd]


def clean_env(monkeypatch):
    for k in ENVS: monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("n_upd", [1, 2])
def test_heterogeneous_group_equals_its_twins(B, n_upd, monkeypatch):
    """P = 5: double DQN / SmoothL1, the fused_ok limit at B = 64 with a hard update, AdamW with a ragged row block (B = 17),
    a three-layer net with clip_td_err, and a second seed of the first - twelve group opts with pushes in between."""
    clean_env(monkeypatch)
    want = twins_of_test1(B, n_upd)
    got = run_group(B, hetero(B, n_upd), twelve_opts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")
        assert len(g["losses"]) == 3 and g["n_opts"] == 12
    assert not (got[0]["arenas"]["qnet"] == got[4]["arenas"]["qnet"]).all()   # (the two seeds of one config do differ)


@pytest.mark.parametrize("n_upd", [1, 2])
def test_global_memory_form_same_bits(B, n_upd, monkeypatch):
    """the group entry of k_dqn_mlp_step (BDR_NO_MLP_LDS=1) against the twins stepped WITHOUT it"""
    clean_env(monkeypatch)
    want = twins_of_test1(B, n_upd)
    monkeypatch.setenv("BDR_NO_MLP_LDS", "1")
    got = run_group(B, hetero(B, n_upd), twelve_opts)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")


def test_member_calls_mix_with_group_calls(B, monkeypatch):
    """group opt, member c alone through bdr_agent_opt, group opt - against the twins run in that same order"""
    clean_env(monkeypatch)
    def sched(step, push):
        step(False); push(20)
        step(False, only=2); step(True, only=2)
        push(20); step(True)
    members = hetero(B, 1)
    want = run_twins(B, members, sched)
    got = run_group(B, members, sched)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")
    assert [g["n_opts"] for g in got] == [2, 2, 4, 2, 2]


def test_steps_without_a_synchronise_in_between(B, monkeypatch):
    """K group opts back to back: the per-step staging ring is rewritten K / depth times while launches are still queued"""
    clean_env(monkeypatch)
    K = max(50, 4 * B.DqnGroup.STAGING_DEPTH)
    def sched(step, push):
        for _ in range(K): step(False)
    members = hetero(B, 1)[:3]
    want = run_twins(B, members, sched)
    got = run_group(B, members, sched)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"member {i}")
        assert g["n_opts"] == K


def three_opts(step, push):
    for _ in range(3): step(False)


def test_a_group_of_one(B, monkeypatch):
    clean_env(monkeypatch)
    members = hetero(B, 1)[:1]
    assert_same(run_group(B, members, three_opts)[0], run_twins(B, members, three_opts)[0])


def test_bound_buffers_and_one_array_of_rows(B, monkeypatch):
    """the Python mirror's cheap forms: opt() on the buffers named last, sample / qvalues on one [n, in_dim] array"""
    clean_env(monkeypatch)
    h = hetero(B, 1)
    members = [h[0], h[1], h[4]]   # one input width
    want = run_twins(B, members, three_opts)
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [Ring(B, c, seed) for c, seed in members]
    with pytest.raises(ValueError):
        g.opt()
    g.opt([r.rb for r in rings]); g.opt(); g.opt()
    g.sync()
    for i, (m, r) in enumerate(zip(g.members, rings)):
        assert_same(state(m, r, []), want[i], f"member {i}")
    rows = np.random.default_rng(2).standard_normal((3, 4)).astype(np.float32)
    for qa, ql, m, row in zip(g.qvalues(rows), g.qvalues(list(rows)), g.members, rows):
        assert (qa == ql).all() and (qa == m.qvalues(row[None])[0]).all()
    for m in g.members: m.eval()
    q = g.qvalues(rows)
    act, info = g.sample(rows, return_info=True)
    for i in range(3):   # eval mode: the greedy action unless the 1 % random branch was taken
        assert info[i]["is_random"] or act[i] == int(np.argmax(q[i])), i
    g.close()
    for r in rings: r.rb.close()


def test_more_members_than_compute_units(B, monkeypatch):
    """P = 260 workgroups on 256 CUs: Mlp[32], B = 8, members differing in their seeds only; twins one at a time"""
    clean_env(monkeypatch)
    members = [(cfg(B, 4, (32,), 2, 8, param_seed=100 + i, tau=0.1), 200 + i) for i in range(260)]
    mk = lambda c, s: Ring(B, c, s, capacity=64, first=40)
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [mk(c, s) for c, s in members]
    for _ in range(3): g.opt([r.rb for r in rings])
    g.sync()
    got = [state(m, r, []) for m, r in zip(g.members, rings)]
    g.close()
    for r in rings: r.rb.close()
    for i, (c, s) in enumerate(members):
        a, ring = B.Dqn.build(c), mk(c, s)
        for _ in range(3): a.opt(ring.rb)
        want = state(a, ring, [])
        a.close(); ring.rb.close()
        assert_same(got[i], want, f"member {i}")
        assert got[i]["n_opts"] == 3


@pytest.mark.parametrize("mode", ["eps_greedy", "softmax", "eval"])
def test_acting_equals_the_twins(B, mode, monkeypatch):
    """50 group.sample calls with opts in between: actions, every bdr_sample_info field and the action values themselves"""
    clean_env(monkeypatch)
    members = hetero(B, 1)[:4]
    def prepare_one(i, a):
        if mode == "eval": a.eval()
        else: a.train()
        a.set_explorer(B.EpsilonGreedy(final_step=20) if mode == "eps_greedy" else B.Softmax(), seed=70 + i)   # (final_step 20: the schedule is crossed)
    obs_rng = np.random.default_rng(8)
    rows = [[obs_rng.standard_normal(c.model_config.q_config.in_dim).astype(np.float32) for c, _ in members] for _ in range(50)]
    # twins
    want_act, want_info, want_q = [], [], []
    for i, (c, seed) in enumerate(members):
        a, ring = B.Dqn.build(c), Ring(B, c, seed)
        prepare_one(i, a)
        acts, infos, qs = [], [], []
        for k in range(50):
            act, info = a.sample(rows[k][i][None], return_info=True)
            acts.append(int(act[0])); infos.append(info)
            if k % 10 == 3: qs.append(a.qvalues(rows[k][i][None])[0])
            if k % 5 == 4: a.opt(ring.rb)
        want_act.append(acts); want_info.append(infos); want_q.append(qs)
        a.close(); ring.rb.close()
    # group
    g = B.DqnGroup.build([c for c, _ in members])
    rings = [Ring(B, c, seed) for c, seed in members]
    for i, m in enumerate(g.members): prepare_one(i, m)
    got_q = [[] for _ in members]
    n_random = 0
    for k in range(50):
        act, info = g.sample(rows[k], return_info=True)
        for i in range(len(members)):
            assert int(act[i]) == want_act[i][k], (k, i)
            assert info[i] == want_info[i][k], (k, i)
            n_random += info[i]["is_random"]
        if k % 10 == 3:
            for i, q in enumerate(g.qvalues(rows[k])): got_q[i].append(q)
        if k % 5 == 4: g.opt([r.rb for r in rings])
    for i in range(len(members)):
        for q, w in zip(got_q[i], want_q[i]):
            assert q.shape == w.shape and (q == w).all(), i
        assert (g.members[i].qvalues(rows[0][i][None])[0] == g.qvalues(rows[0])[i]).all()   # a member's own call, on the group's stream
    if mode == "eps_greedy": assert 0 < n_random < 200
    g.close()
    for r in rings: r.rb.close()


def test_refusals_leave_nothing_behind(B, monkeypatch):
    clean_env(monkeypatch)
    ok = hetero(B, 1)[:2]
    # create
    for bad, word in ((cfg(B, 4, (256, 256), 2, 64), "one-workgroup"),
                      (cfg(B, opt=B.OptimizerConfig.AdamW(1e-3, amsgrad=True)), "amsgrad"),
                      (cfg(B, n_updates_per_opt=2), "n_updates_per_opt")):
        with pytest.raises(B.BdrError) as e:
            B.DqnGroup.build([ok[0][0], bad])
        assert "member 1" in str(e.value) and word in str(e.value), str(e.value)
    # opt
    def sched(step, push):
        step(False); step(True)
    want = run_twins(B, ok, sched)
    g = B.DqnGroup.build([c for c, _ in ok])
    rings = [Ring(B, c, seed) for c, seed in ok]
    bufs = [r.rb for r in rings]
    g.opt(bufs)
    per = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4, per_config=B.PerConfig()), (4,), np.float32)
    r = np.random.default_rng(0)
    per.push(r.standard_normal((40, 4)).astype(np.float32), r.integers(0, 2, (40, 1)).astype(np.int64), r.standard_normal((40, 4)).astype(np.float32),
             np.ones(40, np.float32), np.zeros(40, np.int8), np.zeros(40, np.int8))
    empty = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=700, seed=4), (4,), np.float32)
    for wrong, word in ((per, "prioritized"), (empty, "empty")):
        with pytest.raises(B.BdrError) as e:
            g.opt([bufs[0], wrong])     # member 0's buffer is fine: nothing of it may advance either
        assert "member 1" in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(B.BdrError):
        g.opt([bufs[0], bufs[0]])       # one ring for two members
    with pytest.raises(B.BdrError):
        g.members[1].close()            # the group owns its members
    assert g.members[1].handle is not None
    losses = [rec["loss"] for rec in g.opt_with_record(bufs)]
    for i, (m, ring) in enumerate(zip(g.members, rings)):
        assert_same(state(m, ring, [losses[i]]), want[i], f"member {i}")   # index streams and adam_step were untouched
    g.close()
    per.close(); empty.close()
    for ring in rings: ring.rb.close()
