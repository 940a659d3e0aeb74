"""CandleDqnCnnGroup.sample (bdr_candle_dqn_cnn_group_sample / _sample_members: k_cnn_act_trunk_group and k_cnn_act_head_group, then
every selected member's own explorer) against the float64 forward of tests/candle_dqn_cnn_restatement.py and against the members
acting alone on the image path.  Every member holds its OWN parameters and its own frame stacks: a wrong member index shows up.

Bar (tests/test_gpu_candle_dqn_cnn_act.py): 4 x the largest |float32 restatement - float64 restatement| of the case."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import candle_dqn_cnn_restatement as R  # noqa: E402
import candle_dqn_restatement as RM  # noqa: E402

pytestmark = pytest.mark.gpu
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
# (n_stack, A, n, P, members): one row; a ragged tile with every member; the full tile with a subset
CASES = [(1, 2, 1, 1, None), (4, 6, 3, 3, None), (4, 18, 32, 3, [0, 2])]


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


@functools.lru_cache(maxsize=None)
@R.single_thread
def reference(n_stack, A, n, i):
    """member i of a case: spec, (qnet, qnet_tgt), n frame stacks, the float64 Q rows and the bar - once per session"""
    spec = R.CandleDqnCnnSpec(n_stack, A, adamw=ADAMW)
    pp = spec.init_params(100 * n_stack + A + 1000 * i)
    obs = R.make_batch(spec, n, 7 * n + A + 1000 * i)[0]
    q32, q64 = (R.CandleDqnCnnRestatement(spec, pp[0], pp[0], t).qvalues(obs.astype(np.float32)).astype(np.float64) for t in (torch.float32, torch.float64))
    return spec, pp, obs, q64, 4.0 * float(np.abs(q32 - q64).max())


def load(a, pp, explorer, seed):
    a.set_params(pp[0], "qnet"); a.set_params(pp[1], "qnet_tgt")
    a.set_explorer(explorer, seed=seed)
    return a


def group(B, shape, P, explorers, **kw):
    """P members of one shape, member i with reference(i)'s parameters and explorers[i] seeded 1 + i; and their frame stacks"""
    refs = [reference(*shape, i) for i in range(P)]
    g = B.CandleDqnCnnGroup.build([refs[i][0].to_config(B, 2, device=0, **kw) for i in range(P)])
    for i in range(P): load(g.members[i], refs[i][1], explorers[i], 1 + i).set_act_path("image")   # (the members' OWN calls: bookkeeping)
    return g, [r[2] for r in refs]


def twin(B, shape, i, explorer, **kw):
    spec, pp, obs, _, _ = reference(*shape, i)
    a = load(B.CandleDqn.build(spec.to_config(B, 2, device=0, **kw)), pp, explorer, 1 + i)
    a.set_act_path("image")
    return a, obs


def bookkeeping(a, obs):
    """the member's counters after one more call of its own (which also shows where its explorer stream stands)"""
    act, info = a.sample(obs, return_info=True)
    return act.tolist(), info["eps"], info["is_random"], info["n_samples_act"], info["n_samples_best_act"], a.explorer_state()["n_opts"]


EXPLORERS = lambda B: [B.Softmax(), B.EpsilonGreedy(eps_start=0.5, eps_final=0.02, final_step=50), B.Softmax()]
VERBOSE = dict(train=True, record_verbose_level=2)   # (n_samples_best_act counts at this level)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n_stack,A,n,P,members", CASES)
def test_q_and_the_greedy_action_against_float64(B, n_stack, A, n, P, members):
    sel = list(range(P)) if members is None else members
    for i in sel:
        _, _, _, q64, bar = reference(n_stack, A, n, i)
        top = np.sort(q64, axis=1)
        assert (top[:, -1] - top[:, -2]).min() > 2 * bar, "the seeds leave no row out of the greedy comparison"
        assert RM.CandleDqnExplorer(seed=1 + i).rng.gen_f32() >= np.float32(0.01)   # eval mode: the first call is a greedy one
    g, rows = group(B, (n_stack, A, n), P, [B.Softmax()] * P)
    act = g.sample(rows, members=members)
    for i in range(P):
        if i not in sel:
            assert act[i] is None
            continue
        _, _, _, q64, bar = reference(n_stack, A, n, i)
        q = g.last_q(i, n)
        d = float(np.abs(q.astype(np.float64) - q64).max())
        print((n_stack, A, n, P), "member", i, "|q - q64|", d, "bar", bar)
        assert d <= bar and (act[i] == q64.argmax(1)).all()
    g.close()


def test_group_calls_equal_the_members_own_calls(B):
    """members 0 (Softmax) and 1 (epsilon-greedy) in train mode, twice; member 2 is left out and then acts as if never called"""
    shape = (4, 6, 3)
    g, rows = group(B, shape, 3, EXPLORERS(B), **VERBOSE)
    twins = [twin(B, shape, i, EXPLORERS(B)[i], **VERBOSE)[0] for i in range(3)]
    for call in range(2):
        act = g.sample(rows, members=[0, 1])
        assert act[2] is None
        for i in (0, 1):
            assert (bits(g.last_q(i, 3)) == bits(twins[i].qvalues(rows[i]))).all(), (call, i)
            assert (act[i] == twins[i].sample(rows[i])).all(), (call, i)
            assert g.members[i].explorer_state() == twins[i].explorer_state()
    act = g.sample(rows)
    for i in range(3):
        assert (act[i] == twins[i].sample(rows[i])).all(), i
    for i in range(3):   # the stream, the epsilon counter and both sample counters stand where the twins' stand
        assert bookkeeping(g.members[i], rows[i]) == bookkeeping(twins[i], rows[i]), i
    g.close()
    for t in twins: t.close()


def test_acting_between_rounds(B):
    shape, P = (4, 6, 3), 2
    data = [R.make_batch(reference(*shape, i)[0], 16, 600 + i) for i in range(P)]

    def ring(i):
        rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=100 + i), (reference(*shape, i)[0].row_bytes,), np.uint8, (1,), np.int64)
        obs, a, nxt, rew, term, trunc = data[i]
        rb.push(obs, a.reshape(-1, 1), nxt, rew, term, trunc)
        return rb
    g, rows = group(B, shape, P, [B.Softmax()] * P, train=True)
    bufs = [ring(i) for i in range(P)]
    g.opt(bufs); act = g.sample(rows); g.opt(bufs); g.sync()
    for i in range(P):
        t, _ = twin(B, shape, i, B.Softmax(), train=True)
        rb = ring(i)
        t.opt(rb); want = t.sample(rows[i]); q = t.qvalues(rows[i]); t.opt(rb); t.sync()
        assert (act[i] == want).all() and (bits(g.last_q(i, 3)) == bits(q)).all(), i
        for k in ("qnet", "qnet_tgt"):
            assert g.members[i].get_params(k).tobytes() == t.get_params(k).tobytes(), (i, k)
        t.close(); rb.close()
    g.close()
    for rb in bufs: rb.close()


@pytest.mark.parametrize("P", [1, 3])
def test_two_launches_per_call(B, P):
    g, rows = group(B, (1, 2, 1), P, [B.Softmax()] * P)
    for _ in range(2):
        base = g.kernel_launches
        g.sample(rows)
        assert g.kernel_launches - base == 2 and g.launches_per_round == 17
    g.close()


def test_refusals_leave_everything_where_it_was(B):
    g, rows = group(B, (1, 2, 1), 3, EXPLORERS(B), **VERBOSE)
    many = lambda k: [np.zeros((k, 7056), np.uint8)] * 3
    before = g.kernel_launches
    for kw, match in ((dict(rows=many(0)), "batch size"), (dict(rows=many(33)), "own sample"), (dict(rows=rows, members=[2, 0]), "member 0 .*ascending"),
                      (dict(rows=rows, members=[0, 3]), "member 3 "), (dict(rows=[rows[0], None, rows[2]]), "member 1: null")):
        with pytest.raises(B.BdrError, match=match):
            g.sample(**kw)
        assert g.kernel_launches == before, kw
    for i in range(3):   # nobody drew or counted: every member's next call of its own is a never-called twin's first
        t, _ = twin(B, (1, 2, 1), i, EXPLORERS(B)[i], **VERBOSE)
        assert bookkeeping(g.members[i], rows[i]) == bookkeeping(t, rows[i]), i
        t.close()
    with pytest.raises(NotImplementedError):
        g.evaluate([])
    g.close()
