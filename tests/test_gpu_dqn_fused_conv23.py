"""The fused conv2 + conv3 forward of the split-arithmetic DQN step (csrc/fwd_c23_b3.hpp: one launch per image instead of one launch per
layer) against the two-launch form of the SAME binary, which forward() keeps while the per-kernel profile is enabled.  The fused kernel
promises every output element the accumulation it had (same k order, same six partial products per k-step, one accumulator), so every
check here is bit for bit: activations, Q-values, and the parameters and optimizer state after training.  The fused launch carries the
forwards on the agent's own queue; under the default schedule the target network's forward runs on another queue and keeps the two
launches, under the serial schedule (BDR_SCHED=0) every instance of an update goes through one fused launch."""
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


def make_agent(B, two_launches, **kw):
    kw.setdefault("batch_size", BATCH)
    cfg = B.DqnConfig(model_config=B.DqnModelConfig(q_config=B.AtariCnnConfig(n_stack=4, out_dim=A), opt_config=B.OptimizerConfig.Adam(1e-4)),
                      device=0, critic_loss="SmoothL1", **kw)
    a = B.Dqn.build(cfg)
    a.train()
    if two_launches:
        a.profile_enable(True)
    return a


def both_forms(fn):
    """fn(two_launches) with the profile enabled (one launch per layer) and without (fused) -> (reference, got)"""
    return fn(True), fn(False)


def assert_same(got, ref):
    assert len(got) == len(ref)
    for k, (x, y) in enumerate(zip(got, ref)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k
    assert all(np.isfinite(np.asarray(x, np.float64)).all() for x in got)


def state(a):
    return [a.get_params("qnet"), a.get_params("qnet_tgt"), a.get_params("exp_avg")]


def rows(rng, n):
    return (rng.integers(0, 256, (n, *OBS), dtype=np.uint8), rng.integers(0, A, n).astype(np.int64), rng.integers(0, 256, (n, *OBS), dtype=np.uint8),
            rng.standard_normal(n).astype(np.float32), np.zeros(n, np.int8))


def layers(a, n):
    return [a.probe("act_conv2", n * 81 * 64), a.probe("act_conv3", n * 49 * 64), a.probe("q_pred_all", n * A), a.probe("q_next_all", n * A)]


def make_ring(B, per=False):
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=RING, seed=42, per_config=B.PerConfig(n_opts_final=40) if per else None), OBS, "uint8")
    rb.fill_synthetic(RING, seed=3, kind=0, n_actions=A)
    return rb


@pytest.mark.parametrize("n,double_dqn,serial", [(1, False, False), (3, False, False), (3, True, False), (3, True, True)])
def test_layer_outputs_are_the_same_words(B, n, double_dqn, serial, monkeypatch):
    """a2 and a3 of an update, word for word.  A workgroup of the fused kernel owns one image (grid = images x instances, no stride over
    images): one image, and an odd count; with double DQN one launch carries two instances, and under the serial schedule three (both
    parameter sets' planes).  The Q rows of the instances the probes of a2 / a3 do not show follow from their a3."""
    if serial:
        monkeypatch.setenv("BDR_SCHED", "0")
    else:
        monkeypatch.delenv("BDR_SCHED", raising=False)
    from oracle import torch_ref as T
    p0, p1 = T.init_params(T.cnn_shapes(A), 21), T.init_params(T.cnn_shapes(A), 22)

    def run(two_launches):
        a = make_agent(B, two_launches, double_dqn=double_dqn)
        a.set_params(p0, "qnet"); a.set_params(p1, "qnet_tgt")
        a.update_on_batch(*rows(np.random.default_rng(100 + n), n))
        out = layers(a, n)
        a.close()
        return out

    ref, got = both_forms(run)
    for y in ref[:2]:   # the ReLU epilogue ran on both sides
        assert (y == 0).any() and (y > 0).any()
    assert_same(got, ref)


def test_qvalues_rows_outside_an_update(B):
    """qvalues on 24 rows is the training forward outside an update, with a row count that is a multiple of nothing."""
    from oracle import torch_ref as T
    p0 = T.init_params(T.cnn_shapes(A), 23)
    obs = np.random.default_rng(7).integers(0, 256, (24, *OBS), dtype=np.uint8)

    def run(two_launches):
        a = make_agent(B, two_launches)
        a.set_params(p0, "qnet")
        out = [a.qvalues(obs).copy()]
        a.close()
        return out

    ref, got = both_forms(run)
    assert np.unique(ref[0]).size > 24
    assert_same(got, ref)


@pytest.mark.parametrize("variant", ["plain", "double_dqn", "prioritized", "serial"])
def test_training_is_bit_identical(B, variant, monkeypatch):
    """20 opt calls with a soft update every third one: the online forward behind the CONV23 join, the target forward on the other queue
    (with prioritized replay behind the tail), two instances per launch with double DQN; under the serial schedule the target network's
    instance is in the fused launch too."""
    if variant == "serial":
        monkeypatch.setenv("BDR_SCHED", "0")
    else:
        monkeypatch.delenv("BDR_SCHED", raising=False)

    def run(two_launches):
        rb = make_ring(B, per=variant == "prioritized")
        a = make_agent(B, two_launches, tau=0.5, soft_update_interval=3, param_seed=5, double_dqn=variant == "double_dqn")
        for _ in range(20):
            a.opt(rb)
        a.sync()
        out = state(a)
        a.close(); rb.close()
        return out

    ref, got = both_forms(run)
    assert not np.array_equal(ref[0], ref[1])   # (the run trained: online and target network differ)
    assert_same(got, ref)


def test_conv_parameter_writers_other_than_the_update(B, tmp_path):
    """set_params, load_params and arena_device_ptr leave the bf16 weight planes stale (cpl_fresh / cpl_escaped); the fused launch sits
    behind the same refresh as the two launches and must read the re-split planes: one update after each writer."""
    def run(two_launches):
        rng = np.random.default_rng(31)
        rb = make_ring(B)
        a = make_agent(B, two_launches, tau=0.5, soft_update_interval=2, param_seed=6)
        for _ in range(3):
            a.opt(rb)
        out = []

        def step():
            a.update_on_batch(*rows(rng, 5))
            out.extend(layers(a, 5) + state(a))

        pq, pt = a.get_params("qnet"), a.get_params("qnet_tgt")
        a.set_params(pt * np.float32(1.25), "qnet"); a.set_params(pq * np.float32(0.75), "qnet_tgt")
        step()
        d = str(tmp_path / ("two" if two_launches else "fused"))
        a.save_params(d)
        a.opt(rb)
        a.load_params(d)
        step()
        a.arena_device_ptr("qnet"); a.arena_device_ptr("qnet_tgt")   # from here on the planes are re-split before every forward
        step()
        step()
        a.close(); rb.close()
        return out

    ref, got = both_forms(run)
    assert_same(got, ref)
