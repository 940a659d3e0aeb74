"""k_dense_act (csrc/dense_act.hpp): Policy::sample of the IQL, AWAC and BC agents in one launch - raw rows, the normaliser, every
layer, the action - against the layer-by-layer path of the same agent.

Bit identity is derived, not measured: both paths form every 32 x 32 tile of every layer through dense_small_tile[_pre] /
dense_small_sum (dense.hpp) and run the same element code afterwards, so every comparison between the two paths is `==` on the
raw bits.  Two agents are built from the same parameters and seed, one on each path.  The float32 restatements' `sample`
(tests/iql_restatement.py and siblings) are compared within 1e-5, the bar of tests/test_gpu_iql.py::test_iql_sample."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
import awac_restatement as RA  # noqa: E402
import bc_restatement as RB  # noqa: E402
import iql_restatement as RI  # noqa: E402

ROWS = (1, 31, 32, 33, 65)
# the smallest shapes that reach every branch of the tile walk and the LDS plan: (obs, act, hidden)
SHAPES = {
    "one_tile": (10, 4, (32,)),               # one tile per layer, one k-chunk
    "pen": (45, 24, (256, 256, 256)),         # the pen shape
    "ragged": (70, 40, (96, 320)),            # Kp = 128; a 320-wide reduction (k-slice 80 = 64 + 16: the chunk loop's second pass, no prefetch);
                                              # two action column tiles; layer widths - and so the ping-pong strides - differ
    "widest": (19, 4, (512,)),                # the largest width the LDS plan admits (one team)
}
KINDS = ("iql", "awac", "bc")


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def make(B, kind, shape, path, seed=21, train=False, params=None, **spec_kw):
    """(agent on `path`, its restatement, its actor / policy parameter vector)"""
    O, A, hidden = shape
    if kind == "iql":
        spec = RI.IqlSpec(O, A, (8,), tuple(hidden), (8,), **spec_kw)
        p = list(spec.init_params(6))
        if params is not None:
            p[0] = params
        a = B.Iql.build(spec.to_config(B, 4, device=0, seed=seed, train=train))
        a.set_params(p[0], "actor")
        ref = RI.IqlRestatement(spec, *p)
        sample = lambda obs, z=None: np.asarray(ref.sample(obs, z))
    elif kind == "awac":
        spec = RA.AwacSpec(O, A, tuple(hidden), (8,), **spec_kw)
        p = list(spec.init_params(6))
        if params is not None:
            p[0] = params
        a = B.Awac.build(spec.to_config(B, 4, device=0, seed=seed, train=train))
        a.set_params(p[0], "actor")
        ref = RA.AwacRestatement(spec, *p)
        sample = lambda obs, z=None: np.asarray(ref.sample(obs, z))
    else:
        spec = RB.BcSpec(O, A, tuple(hidden), **spec_kw)
        p = [spec.init_params(6) if params is None else params]
        a = B.Bc.build(spec.to_config(B, 4, device=0, seed=seed))
        a.set_params(p[0])
        ref = RB.BcRestatement(spec, p[0])
        sample = lambda obs, z=None: np.asarray(ref.sample(obs))
    a.set_act_path(path)
    return a, sample, p[0]


def pair(B, kind, shape, **kw):
    f, sample, p = make(B, kind, shape, "fused", **kw)
    l, _, _ = make(B, kind, shape, "layers", **kw)
    return f, l, sample, p


def obs_rows(n, O, seed=0):
    return np.random.default_rng(1000 * n + seed).standard_normal((n, O)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- fused == layers, eval mode
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", KINDS)
def test_eval_actions_have_the_bits_of_the_layer_path(B, kind, shape):
    f, l, ref, _ = pair(B, kind, SHAPES[shape])
    for n in ROWS:
        obs = obs_rows(n, SHAPES[shape][0])
        af, al = f.sample(obs), l.sample(obs)
        assert af.shape == (n, SHAPES[shape][1]) and np.isfinite(af).all()
        assert (bits(af) == bits(al)).all(), (kind, shape, n, np.abs(af - al).max())
        assert np.abs(af - ref(obs)).max() < 1e-5, (kind, shape, n, np.abs(af - ref(obs)).max())
    f.close(); l.close()


def test_many_rows_take_the_staged_copy_and_the_plain_result_copy(B):
    """2049 rows of the pen shape: 65 row blocks (more workgroups than one wave of them per XCD), host rows beyond the pinned
    area (a staged copy) and more result floats than the pinned result area holds"""
    f, l, ref, _ = pair(B, "iql", SHAPES["pen"])
    obs = obs_rows(2049, 45)
    af = f.sample(obs)
    assert (bits(af) == bits(l.sample(obs))).all()
    assert np.abs(af - ref(obs)).max() < 1e-5
    f.close(); l.close()


# ---------------------------------------------------------------------------------------------------------- train mode: one stream of draws
@pytest.mark.parametrize("kind", ("iql", "awac"))
def test_train_mode_fused_and_layer_calls_share_one_stream_of_draws(B, kind):
    shape = SHAPES["pen"]
    x, ref, _ = make(B, kind, shape, "fused", train=True)
    y, _, _ = make(B, kind, shape, "layers", train=True)
    z, _, _ = make(B, kind, shape, "layers", train=True)
    got, want, rows = [], [], []
    for call, (path, n) in enumerate((("fused", 33), ("layers", 1), ("fused", 65))):
        obs = obs_rows(n, shape[0], seed=call)
        x.set_act_path(path)
        got.append(x.sample(obs)); want.append(y.sample(obs)); rows.append(obs)
    for g, w in zip(got, want):
        assert (bits(g) == bits(w)).all()
    # draw_noise on an untouched twin replays what the three calls drew, in order: n * A draws per call
    for g, obs in zip(got, rows):
        zz = z.draw_noise(obs.shape[0] * shape[1]).reshape(obs.shape[0], shape[1])
        assert np.abs(g - ref(obs, zz)).max() < 1e-5
    # ... and the next draw of all three agents is the same one
    dx, dy, dz = x.draw_noise(8), y.draw_noise(8), z.draw_noise(8)
    assert (dx == dy).all() and (dy == dz).all()
    # eval mode draws nothing
    x.eval(); y.eval()
    x.sample(rows[0]); y.sample(rows[0])
    assert (x.draw_noise(4) == y.draw_noise(4)).all()
    x.close(); y.close(); z.close()


# ---------------------------------------------------------------------------------------------------------- the limits, saturated
@pytest.mark.parametrize("train", (False, True))
@pytest.mark.parametrize("limit", ("Clamp", "Tanh"))
def test_clamp_and_tanh_limits_with_saturating_means(B, limit, train):
    O, A, hidden = shape = SHAPES["one_tile"]
    kw = dict(action_limit=limit, action_scale=1.5, action_min=-0.3, action_max=0.4)
    p = RI.IqlSpec(O, A, (8,), tuple(hidden), (8,), **kw).init_params(6)[0].copy()
    p[-2 * A:-A] = [50.0, -50.0, 50.0, -50.0]      # the last layer's bias: means far beyond either limit
    f, l, ref, _ = pair(B, "iql", shape, params=p, train=train, **kw)
    for n in (1, 33):
        obs = obs_rows(n, O)
        af = f.sample(obs)
        assert (bits(af) == bits(l.sample(obs))).all()
        want = np.array([0.4, -0.3, 0.4, -0.3] if limit == "Clamp" else [1.5, -1.5, 1.5, -1.5], np.float32)
        assert (af == want).all(), af[0]          # tanh(+-50 +- a few std) is +-1 in float32: the scale, exactly
    f.close(); l.close()


# ---------------------------------------------------------------------------------------------------------- BC
@pytest.mark.parametrize("act_out", ["None", "ReLU", "Tanh", "Sigmoid"])
def test_bc_continuous_with_each_output_activation(B, act_out):
    shape = SHAPES["ragged"]
    f, l, ref, _ = pair(B, "bc", shape, activation_out=act_out)
    for n in (1, 33):
        obs = obs_rows(n, shape[0])
        af = f.sample(obs)
        assert af.dtype == np.float32 and (bits(af) == bits(l.sample(obs))).all()
        assert np.abs(af - ref(obs)).max() < 1e-5
    f.close(); l.close()


@pytest.mark.parametrize("act_out", ["None", "ReLU"])
def test_bc_discrete_takes_the_argmax_and_the_lowest_index_among_exact_ties(B, act_out):
    O, A, hidden = shape = (10, 6, (32, 32))
    spec = RB.BcSpec(O, A, hidden, act_out, action_type="Discrete")
    p = spec.init_params(6)
    f, l, ref, _ = pair(B, "bc", shape, activation_out=act_out, action_type="Discrete")
    obs = obs_rows(65, O)
    i_f, i_l = f.sample(obs), l.sample(obs)
    assert i_f.dtype == np.int64 and i_f.shape == (65,) and (i_f == i_l).all()
    f.close(); l.close()
    # exact ties: an all-zero last layer makes every output 0 - index 0; with the bias [0, 1, 1, .5, 1, 0] the maximum is shared by
    # 1, 2 and 4 - index 1
    last = 32 * A + A
    for bias, want in ((np.zeros(A), 0), (np.array([0, 1, 1, .5, 1, 0]), 1)):
        q = p.copy()
        q[-last:] = 0.0
        q[-A:] = bias
        f, l, _, _ = pair(B, "bc", shape, params=q, activation_out=act_out, action_type="Discrete")
        for n in (1, 33):
            i_f = f.sample(obs[:n])
            assert (i_f == want).all() and (l.sample(obs[:n]) == want).all()
        f.close(); l.close()


# ---------------------------------------------------------------------------------------------------------- eligibility
@pytest.mark.parametrize("kind", KINDS)
def test_a_network_wider_than_the_lds_plan_keeps_the_layer_path(B, kind):
    shape = (19, 4, (544,))                       # padded to 576 > 512
    a, ref, _ = make(B, kind, shape, "default")
    with pytest.raises(B.BdrError, match="512"):
        a.set_act_path("fused")
    obs = obs_rows(33, 19)
    assert np.abs(a.sample(obs) - ref(obs)).max() < 1e-5      # the refused request left the agent on its path
    a.set_act_path("layers")
    assert np.abs(a.sample(obs) - ref(obs)).max() < 1e-5
    a.close()


def test_agents_without_the_kernel_refuse_the_fused_path(B):
    from border_amd import _lib
    a = B.Sac.build(B.SacConfig(obs_dim=8, act_dim=2, device=0, batch_size=4))
    assert _lib.lib().bdr_agent_set_act_path(a.handle, _lib.BDR_ACT_PATH_FUSED) == 1      # BDR_ERR_INVALID
    assert _lib.lib().bdr_agent_set_act_path(a.handle, _lib.BDR_ACT_PATH_LAYERS) == 0
    out = np.zeros(2, np.float32)
    row = np.zeros(8, np.float32)
    assert _lib.lib().bdr_agent_sample_raw(a.handle, None, 1, row.ctypes.data, 0, 0, 0, out.ctypes.data, None) == 1
    a.close()


# ---------------------------------------------------------------------------------------------------------- raw rows
def normaliser(B, O):
    """columns whose mean is far above their spread (1000 + 0.01 k, as tests/test_dataset_host.py): x - mean cancels almost every bit"""
    k = np.arange(O)
    mean = (1000.0 + 0.01 * k).astype(np.float32)
    std = (0.5 + 0.25 * (k % 5)).astype(np.float32)
    return B.ObsNormalizer(O, 0).set(mean, std), mean, std


def raw_rows(n, O, mean, std, dtype):
    x = mean.astype(np.float64) + std.astype(np.float64) * np.random.default_rng(n).standard_normal((n, O))
    x[-1, -1] = 1000.0000001 + 0.01 * (O - 1)     # not representable in float32, in the last column of the last row (of a ragged block for n = 33)
    assert np.float64(np.float32(x[-1, -1])) != x[-1, -1]
    return x.astype(dtype)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("kind", KINDS)
def test_raw_rows_with_a_normaliser_on_either_path(B, kind, dtype):
    import torch
    O, A, hidden = shape = SHAPES["pen"]
    f, l, ref, _ = pair(B, kind, shape)
    norm, mean, std = normaliser(B, O)
    for n in (1, 33):
        x = raw_rows(n, O, mean, std, dtype)
        z = (x.astype(np.float32) - mean) / std                   # two separately rounded float32 operations: the element contract
        assert z.dtype == np.float32 and (bits(z) == bits(norm.apply(x))).all()
        want = l.sample(z)
        for a in (f, l):
            assert (bits(a.sample_raw(x, norm)) == bits(want)).all(), (kind, dtype, n)
        assert np.abs(want - ref(z)).max() < 1e-5
        # device rows, a stride wider than the row, the gap poisoned
        wide = torch.full((n, O + 3), float("nan"), dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
        wide[:, :O] = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        for a in (f, l):
            got = a.sample_raw_device(wide.data_ptr(), n, (O + 3) * x.itemsize, dtype, norm)
            assert (bits(got) == bits(want)).all(), (kind, dtype, n)
        # without a normaliser the rows are only rounded to float32
        for a in (f, l):
            assert (bits(a.sample_raw(x)) == bits(l.sample(x.astype(np.float32)))).all()
    f.close(); l.close(); norm.close()


def test_raw_rows_argument_checks(B):
    O, A, hidden = shape = SHAPES["one_tile"]
    a, _, _ = make(B, "iql", shape, "fused")
    other = B.ObsNormalizer(O + 1, 0).set(np.zeros(O + 1, np.float32), np.ones(O + 1, np.float32))
    with pytest.raises(B.BdrError, match="dim"):
        a.sample_raw(np.zeros((1, O)), other)
    unfinished = B.ObsNormalizer(O, 0)
    with pytest.raises(B.BdrError, match="statistics"):
        a.sample_raw(np.zeros((1, O)), unfinished)
    a.close(); other.close(); unfinished.close()


# ---------------------------------------------------------------------------------------------------------- profile
def test_the_fused_path_is_one_launch_per_call(B):
    shape = SHAPES["pen"]
    f, l, _, _ = pair(B, "iql", shape)
    obs = obs_rows(1, shape[0])
    for a in (f, l):
        a.profile_enable(True)
        a.sample(obs); a.sample(obs)
    names_f, names_l = [k for k, _ in f.profile_read()], [k for k, _ in l.profile_read()]
    assert names_f == ["dense_act"]
    assert names_l == ["pi_fwd"] * 4 + ["sample_pack"]          # four layers, then the sample kernel
    assert f.profile_read()[0][1] > 0.0                           # the bracket was timed
    f.close(); l.close()
