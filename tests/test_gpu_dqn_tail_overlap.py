"""The overlapped tail of the DQN update on the flag-ordered schedule: conv2 dW and the conv2 / conv3 optimizer
pass run on the weight-gradient queue beside conv1 dW, conv1's optimizer pass and the NEXT update's conv1 forward on the dX queue.
After such an update "the agent's stream has drained" no longer means "the parameters are final" - a pending join is flushed in front
of everything that touches them.  Every check here is bit for bit against the serial schedule (BDR_SCHED=0) on the same seeds: no
kernel's arithmetic or reduction order differs, so any difference is a race between the queues."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OBS = (4, 1, 84, 84)
RING, BATCH, A = 2000, 32, 6


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def make_agent(B, **kw):
    kw.setdefault("batch_size", BATCH)
    cfg = B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.AtariCnnConfig(n_stack=4, out_dim=A), opt_config=B.OptimizerConfig.Adam(1e-4)),
                      device=0, critic_loss="SmoothL1", **kw)
    a = B.Dqn.build(cfg)
    a.train()
    return a


def make_ring(B, per=False, seed=42):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=RING, seed=seed, per_config=B.PerConfig(n_opts_final=40) if per else None), OBS, "uint8")
    rb.fill_synthetic(RING, seed=3, kind=0, n_actions=A)
    return rb


def both_schedules(fn):
    """fn() under the serial schedule and under the default one -> (reference, got)"""
    out = []
    for sched in ("0", None):
        if sched is None:
            os.environ.pop("BDR_SCHED", None)
        else:
            os.environ["BDR_SCHED"] = sched
        try:
            out.append(fn())
        finally:
            os.environ.pop("BDR_SCHED", None)
    return out


def assert_same(got, ref):
    assert len(got) == len(ref)
    for k, (x, y) in enumerate(zip(got, ref)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x, y), k
    assert all(np.isfinite(np.asarray(x, np.float64)).all() for x in got)


def state(a):
    return [a.get_params("qnet"), a.get_params("qnet_tgt"), a.get_params("exp_avg")]


@pytest.mark.parametrize("variant", ["plain", "two_updates_per_opt", "double_dqn", "prioritized"])
def test_training_is_bit_identical_to_the_serial_schedule(B, variant):
    """~60 opt calls with a soft update every third one (a track follows a pending join many times); with two updates per opt, with
    double DQN (a second online instance in front of the join) and with prioritized replay (gather and target forward on the
    weight-gradient queue, behind the tail)."""
    kw = dict(tau=0.5, soft_update_interval=3, param_seed=5)
    if variant == "two_updates_per_opt":
        kw["n_updates_per_opt"] = 2
    if variant == "double_dqn":
        kw["double_dqn"] = True

    def run():
        rb = make_ring(B, per=variant == "prioritized")
        a = make_agent(B, **kw)
        for _ in range(60 if variant != "two_updates_per_opt" else 30):
            a.opt(rb)
        a.sync()
        out = state(a)
        a.close(); rb.close()
        return out

    ref, got = both_schedules(run)
    assert not np.array_equal(ref[0], ref[1])   # (the run trained: online and target network differ)
    assert_same(got, ref)


def _rows(rng, n):
    return (rng.integers(0, 256, (n, *OBS), dtype=np.uint8), rng.integers(0, A, n).astype(np.int64), rng.integers(0, 256, (n, *OBS), dtype=np.uint8),
            rng.standard_normal(n).astype(np.float32), np.zeros(n, np.int8))


@pytest.mark.parametrize("api", ["get_params", "qvalues", "set_params", "save_load", "opt_with_record", "update_on_batch", "close"])
def test_api_call_directly_after_opt_sees_the_finished_update(B, api, tmp_path):
    """opt() leaves the conv2 / conv3 optimizer pass running on the other queue.  An entry point called right behind it, with no sync
    between, must see the finished parameters of that update, and training must continue to the same bits."""
    def run():
        rng = np.random.default_rng(17)
        rb = make_ring(B)
        a = make_agent(B, tau=0.5, soft_update_interval=4, param_seed=6)
        p0 = a.get_params("qnet")
        out = []
        for _ in range(7):
            a.opt(rb)
        if api == "get_params":
            out.append(a.get_params("qnet"))
        elif api == "qvalues":
            out.append(a.qvalues(rng.integers(0, 256, (3, *OBS), dtype=np.uint8)).copy())
            a.opt(rb)
            out.append(a.qvalues(rng.integers(0, 256, (40, *OBS), dtype=np.uint8)).copy())   # (the training kernels' forward)
        elif api == "set_params":
            a.set_params(p0 * np.float32(0.999), "qnet")
            out.append(a.get_params("qnet"))
        elif api == "save_load":
            d = str(tmp_path / f"ck{len(os.listdir(tmp_path))}")
            a.save_params(d)
            a.opt(rb)
            a.load_params(d)
            out.append(a.get_params("qnet"))
        elif api == "opt_with_record":
            out.append(np.float32(a.opt_with_record(rb)["loss"]))
            out.append(a.get_params("qnet"))
        elif api == "update_on_batch":
            out.append(np.float32(a.update_on_batch(*_rows(rng, 5))["loss"]))
            out.append(a.get_params("qnet"))
        elif api == "close":
            a.close()                                  # work of the last update is still in flight on both queues
            a = make_agent(B, tau=0.5, soft_update_interval=4, param_seed=7)
        for _ in range(6):
            a.opt(rb)
        a.sync()
        out += state(a)
        a.close(); rb.close()
        return out

    ref, got = both_schedules(run)
    assert_same(got, ref)


def test_two_agents_alternating_on_one_ring(B):
    """Flags and the pending join are per agent: two agents that draw from one ring in turn each reach the serial schedule's bits."""
    def run():
        rb = make_ring(B)
        a = make_agent(B, tau=0.5, soft_update_interval=3, param_seed=8)
        b = make_agent(B, tau=1.0, soft_update_interval=2, param_seed=9, batch_size=16)
        for _ in range(20):
            a.opt(rb)
            b.opt(rb)
        out = state(b) + state(a)                      # (no sync: get_params is the first call behind the last opt)
        a.close(); b.close(); rb.close()
        return out

    ref, got = both_schedules(run)
    assert_same(got, ref)
