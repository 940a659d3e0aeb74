"""bdr_replay_push_device_frames: the device push of the single-frame store (bdr_replay_config::frame_stack > 0).  The frames an
incoming stack shares are found by comparing the rows in HBM (k_frame_eq), the host runs the sharing rule of frame_share.hpp on
the answers, and the new frames are copied inside HBM (k_frame_scatter).  Bar: after the call the buffer is exactly what
bdr_replay_push leaves after the same bytes as host rows - rows, cursor, size, PER priorities, frames used - whatever the mix
of host and device pushes, and a store that runs out of frames fails at the same transition with the same state."""
import numpy as np
import pytest

from tests.test_gpu_device_actor import ROW, _Emulator, _cnn, _frames

pytestmark = pytest.mark.gpu
SHAPE = (4, 1, 84, 84)


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def _same_rows(a, b, n):
    for x, y in zip(a.read_rows(0, n), b.read_rows(0, n)):
        assert (x.view(np.uint8) == y.view(np.uint8)).all()


def _same_batches(a, b, times, size, per=False):
    for _ in range(times):
        g, w = a.batch(size), b.batch(size)
        assert g.ix_sample.tolist() == w.ix_sample.tolist() and (g.obs == w.obs).all() and (g.next_obs == w.next_obs).all()
        assert (g.act == w.act).all() and (g.reward.view(np.uint32) == w.reward.view(np.uint32)).all()
        assert (g.is_terminated == w.is_terminated).all() and (g.is_truncated == w.is_truncated).all()
        if per:
            assert (g.weight.view(np.uint32) == w.weight.view(np.uint32)).all()


# ------------------------------------------------------------------------------------------------ 1. parity, Atari shape
@pytest.mark.parametrize("per", [False, True])
def test_device_push_equals_the_host_push_on_atari_stacks(B, per):
    """The loop of test_push_device_writes_the_ring_bit_for_bit_like_the_host_push over three buffers: single-frame store / host
    push, single-frame store / device push, plain ring / push_device.  frame_bytes 7056 = 441 vectors: a ragged loop for 256 threads."""
    rng = np.random.default_rng(11)
    n_envs, cap = 6, 20
    prep = B.AtariPreprocessor(n_envs)
    ixs = np.arange(n_envs)
    prep.reset_device(ixs, _frames(rng, n_envs))
    mk = lambda fs: B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=42, per_config=B.PerConfig() if per else None, frame_stack=fs,
                                                                    frame_capacity=256 if fs else 0), SHAPE, np.uint8)
    rh, rd, rp = mk(4), mk(4), mk(0)
    pushed = 0
    for step in range(9):   # 45 transitions into 20 slots: the ring wraps twice, pushes straddle the end
        obs = prep.obs(ixs)
        prep.step_device(ixs, _frames(rng, n_envs), _frames(rng, n_envs))
        nobs = prep.obs(ixs)
        act = rng.integers(0, 6, (n_envs, 1)).astype(np.int64)
        rew = rng.standard_normal(n_envs).astype(np.float32)
        term = (rng.random(n_envs) < 0.2).astype(np.int8); trunc = (rng.random(n_envs) < 0.1).astype(np.int8)
        sl, stride = (slice(0, n_envs, 2), 2 * ROW) if step % 3 == 2 else (slice(None), ROW)   # every third push ragged: rows with a stride
        rh.push(obs[sl], act[sl], nobs[sl], rew[sl], term[sl], trunc[sl])
        rd.push_device_frames(prep.device_prev_stacks(), stride, act[sl], prep.device_stacks(), stride, rew[sl], term[sl], trunc[sl])
        rp.push_device(prep.device_prev_stacks(), stride, act[sl], prep.device_stacks(), stride, rew[sl], term[sl], trunc[sl])
        pushed += len(rew[sl])
        assert len(rh) == len(rd) == len(rp) and rh.head == rd.head == rp.head
        assert rh.frames_used() == rd.frames_used()
    print(f"frames_used, {n_envs} environments, {pushed} transitions: {rd.frames_used()[0]}")
    _same_rows(rh, rd, cap); _same_rows(rp, rd, cap)
    for _ in range(5):
        bh, bd, bp = rh.batch(8), rd.batch(8), rp.batch(8)
        for w in (bh, bp):
            assert w.ix_sample.tolist() == bd.ix_sample.tolist() and (w.obs == bd.obs).all() and (w.next_obs == bd.next_obs).all()
            assert (w.act == bd.act).all() and (w.reward == bd.reward).all() and (w.is_terminated == bd.is_terminated).all()
            assert (w.is_truncated == bd.is_truncated).all()
            if per:
                assert (w.weight == bd.weight).all()
    rh.close(); rd.close(); rp.close(); prep.close()


def test_one_environment_costs_one_frame_per_transition(B):
    """One continuing chain: the host rule allocates the reset stack once and then one frame per transition, so frames_used is
    at most transitions + k - and the device push's count is the host twin's."""
    rng = np.random.default_rng(5)
    cap, steps, k = 20, 30, 4
    prep = B.AtariPreprocessor(1)
    ixs = np.arange(1)
    prep.reset_device(ixs, _frames(rng, 1))
    mk = lambda fs: B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=42, frame_stack=fs), SHAPE, np.uint8)
    rh, rd, rp = mk(k), mk(k), mk(0)
    for step in range(steps):
        obs = prep.obs(ixs)
        prep.step_device(ixs, _frames(rng, 1), _frames(rng, 1))
        nobs = prep.obs(ixs)
        act = rng.integers(0, 6, (1, 1)).astype(np.int64)
        rew = rng.standard_normal(1).astype(np.float32)
        fl = np.zeros(1, np.int8)
        rh.push(obs, act, nobs, rew, fl, fl)
        rd.push_device_frames(prep.device_prev_stacks(), ROW, act, prep.device_stacks(), ROW, rew, fl, fl)
        rp.push_device(prep.device_prev_stacks(), ROW, act, prep.device_stacks(), ROW, rew, fl, fl)
        assert len(rh) == len(rd) and rh.head == rd.head and rh.frames_used() == rd.frames_used()
    used = rd.frames_used()[0]
    print(f"frames_used, 1 environment, {steps} transitions: {used}")
    assert used == rh.frames_used()[0] and used <= steps + k
    _same_rows(rh, rd, cap); _same_rows(rp, rd, cap)
    _same_batches(rh, rd, 5, 8)
    rh.close(); rd.close(); rp.close(); prep.close()


# ------------------------------------------------------------------------------------------------ 2. the comparison's edges
def _chain(rng, n, k, fb, first=None):
    """n transitions of one continuing episode: obs_s = next_{s-1}, next_s = a new frame shifted into obs_s.  -> obs, next [n, k, fb]"""
    stack = rng.integers(0, 256, (k, fb), dtype=np.uint8) if first is None else first
    obs, nxt = [], []
    for _ in range(n):
        obs.append(stack.copy())
        stack = np.concatenate([rng.integers(0, 256, (1, fb), dtype=np.uint8), stack[:-1]])
        nxt.append(stack.copy())
    return np.stack(obs), np.stack(nxt)


def _side(rng, n):
    return rng.integers(0, 6, (n, 1)).astype(np.int64), rng.standard_normal(n).astype(np.float32), (rng.random(n) < 0.2).astype(np.int8), np.zeros(n, np.int8)


def _push_dev(rb, obs, nxt, act, rew, term, trunc):
    """push_device_frames of host arrays [n, k, fb]: through torch device tensors"""
    import torch
    n = len(obs)
    o = torch.from_numpy(np.ascontiguousarray(obs.reshape(n, -1))).to("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(nxt.reshape(n, -1))).to("cuda:0")
    torch.cuda.synchronize()
    stride = o.shape[1]
    rb.push_device_frames(o.data_ptr(), stride, act, x.data_ptr(), stride, rew, term, trunc)


def _twins(B, k, fb, cap=8, frame_capacity=0, per=False):
    mk = lambda: B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=3, frame_stack=k, frame_capacity=frame_capacity,
                                                                 per_config=B.PerConfig() if per else None), (k, fb), np.uint8)
    return mk(), mk()


def _crafted(B, k, fb, prefix, rows, seed):
    """prefix (a host push on both twins: it becomes the store's last next_obs), then `rows` through the host push on one twin and the
    device push on the other.  Rows read back bit for bit, frames_used equal.  -> frames_used"""
    rng = np.random.default_rng(seed)
    rh, rd = _twins(B, k, fb)
    n0, n = len(prefix[0]), len(rows[0])
    s0, s1 = _side(rng, n0), _side(rng, n)
    rh.push(prefix[0], s0[0], prefix[1], *s0[1:]); rd.push(prefix[0], s0[0], prefix[1], *s0[1:])
    rh.push(rows[0], s1[0], rows[1], *s1[1:])
    _push_dev(rd, rows[0], rows[1], *s1)
    assert len(rh) == len(rd) == n0 + n and rh.head == rd.head
    assert rh.frames_used() == rd.frames_used()
    got = rd.read_rows(0, n0 + n)
    assert (got[0][n0:].reshape(n, k, fb) == rows[0]).all() and (got[2][n0:].reshape(n, k, fb) == rows[1]).all()
    _same_rows(rh, rd, n0 + n)
    used = rd.frames_used()[0]
    rh.close(); rd.close()
    return used


@pytest.mark.parametrize("fb", [16, 16 * 257, 7056])
def test_one_flipped_byte_is_seen_wherever_it_is(B, fb):
    """Stacks that share everything (one continuing episode of 1 + 3 transitions: 4 + 4 frames), then ONE byte flipped - the first
    byte of a frame, the last, the bytes on both sides of the first and of the last 16-byte vector boundary - in the newest obs
    frame, the oldest obs frame, a shifted next_obs frame, or the frame the store holds as the last next_obs.  frame_bytes: one
    vector, one more than a block of 256 threads, the Atari frame (441 vectors)."""
    k = 4
    rng = np.random.default_rng(fb)
    obs, nxt = _chain(rng, 4, k, fb)
    prefix, rows = (obs[:1], nxt[:1]), (obs[1:], nxt[1:])
    base = _crafted(B, k, fb, prefix, rows, 1)
    assert base == k + 4                                  # the first stack, then one frame per transition
    positions = sorted({p for p in (0, 15, 16, fb - 17, fb - 16, fb - 1) if 0 <= p < fb})
    for where in ("obs newest", "obs oldest", "next shifted", "store"):
        for p in positions:
            o, x, po, px = rows[0].copy(), rows[1].copy(), prefix[0].copy(), prefix[1].copy()
            if where == "obs newest": o[1, 0, p] ^= 0x40
            elif where == "obs oldest": o[1, k - 1, p] ^= 0x01
            elif where == "next shifted": x[1, 2, p] ^= 0x80
            else: px[0, 1, p] ^= 0x08                    # obs of the first device-pushed transition no longer continues the store
            used = _crafted(B, k, fb, (po, px), (o, x), 1)
            assert used > base, (where, p)               # the flip costs frames: it was seen (how many: the host twin's count)


def test_equal_neighbouring_frames_are_stored_once(B):
    k, fb = 4, 16 * 257
    rng = np.random.default_rng(8)
    obs, nxt = _chain(rng, 1, k, fb)
    f = rng.integers(0, 256, fb, dtype=np.uint8)
    reset = np.stack([f] * k)                                             # a reset stack: A all equal, next_obs shifts a frame in
    o = np.stack([reset, np.stack([f, f, nxt[0, 0], nxt[0, 0]])])         # and a stack with two pairs of equal neighbours
    x = np.stack([np.concatenate([rng.integers(0, 256, (1, fb), dtype=np.uint8), reset[:-1]]), np.stack([f, f, f, nxt[0, 1]])])
    used = _crafted(B, k, fb, (obs, nxt), (o, x), 2)
    # prefix 4 + 1; reset stack 1 + its new frame 1; then obs {f, nxt00} = 2 new, next_obs {f, nxt01} = 2 new (nothing continues)
    assert used == 5 + 2 + 4


@pytest.mark.parametrize("k", [1, 2, 8])
def test_other_stack_depths(B, k):
    fb = 16
    rng = np.random.default_rng(k)
    obs, nxt = _chain(rng, 3, k, fb)
    o2, x2 = _chain(rng, 3, k, fb, first=np.stack([rng.integers(0, 256, fb, dtype=np.uint8)] * k))   # a reset stack starts a second episode
    rows = (np.concatenate([obs[1:], o2]), np.concatenate([nxt[1:], x2]))
    used = _crafted(B, k, fb, (obs[:1], nxt[:1]), rows, 3)
    assert used == (k + 1) + 2 + (1 + 3)


# ------------------------------------------------------------------------------------------------ 3. mixing
def _episodes(rng, n, k, fb, p_done, state):
    """n transitions the way an Atari environment produces them: a step shifts one new frame in, after an episode end the next
    transition starts from a reset stack (k copies of one frame).  state: {"stack": ...}, carried from call to call"""
    obs, nxt = [], []
    for _ in range(n):
        if state.get("stack") is None:
            state["stack"] = np.stack([rng.integers(0, 256, fb, dtype=np.uint8)] * k)
        obs.append(state["stack"].copy())
        state["stack"] = np.concatenate([rng.integers(0, 256, (1, fb), dtype=np.uint8), state["stack"][:-1]])
        nxt.append(state["stack"].copy())
        if rng.random() < p_done:
            state["stack"] = None
    return np.stack(obs), np.stack(nxt)


def test_host_and_device_pushes_alternate_on_one_buffer(B):
    """host, device, device, host, ... with n = 1 .. 7, twice: 56 transitions into 12 slots.  After a device push the host copy of
    the last next_obs is stale and the next host push fetches it from the frame store; after a host push the device push compares
    against the frames that push wrote."""
    k, fb, cap = 4, 16 * 257, 12
    rng = np.random.default_rng(21)
    state = {}
    chunks = [_episodes(rng, n, k, fb, 0.12, state) for n in list(range(1, 8)) * 2]
    all_host, mixed = _twins(B, k, fb, cap=cap)
    pattern = [False, True, True, False]                 # host, device, device, host, ...
    for c, (o, x) in enumerate(chunks):
        side = _side(rng, len(o))
        all_host.push(o, side[0], x, *side[1:])
        if pattern[c % 4]:
            _push_dev(mixed, o, x, *side)
        else:
            mixed.push(o, side[0], x, *side[1:])
        assert len(all_host) == len(mixed) and all_host.head == mixed.head and all_host.frames_used() == mixed.frames_used()
    _same_rows(all_host, mixed, cap)
    _same_batches(all_host, mixed, 3, 8)
    all_host.close(); mixed.close()


# ------------------------------------------------------------------------------------------------ 4. exhaustion
def test_exhaustion_fails_at_the_same_transition_and_leaves_the_buffer_usable(B):
    k, fb, cap = 4, 7056, 40
    rng = np.random.default_rng(3)
    rh, rd = _twins(B, k, fb, cap=cap, frame_capacity=100, per=True)
    n = 30
    o, x = rng.integers(0, 256, (n, k, fb), dtype=np.uint8), rng.integers(0, 256, (n, k, fb), dtype=np.uint8)   # nothing shares a frame
    side = _side(rng, n)
    with pytest.raises(B.BdrError, match="single-frame store exhausted") as eh:
        rh.push(o, side[0], x, *side[1:])
    with pytest.raises(B.BdrError, match="single-frame store exhausted") as ed:
        _push_dev(rd, o, x, *side)
    assert str(eh.value) == str(ed.value) and ed.value.code == 1
    assert 0 < len(rh) < n and len(rh) == len(rd) and rh.head == rd.head and rh.frames_used() == rd.frames_used()
    m = len(rd)
    _same_rows(rh, rd, m)
    # rows that need no new frame: obs continues the last accepted next_obs, next_obs repeats its newest frame
    o2 = x[m - 1:m]
    x2 = np.stack([np.stack([o2[0, 0], o2[0, 0], o2[0, 1], o2[0, 2]])])
    s2 = _side(rng, 1)
    rh.push(o2, s2[0], x2, *s2[1:])
    _push_dev(rd, o2, x2, *s2)
    assert len(rh) == len(rd) == m + 1 and rh.frames_used() == rd.frames_used()
    _same_rows(rh, rd, m + 1)
    _same_batches(rh, rd, 2, 8, per=True)
    rh.close(); rd.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_buffer_untouched(B):
    import torch
    prep = B.AtariPreprocessor(2)
    side = (np.zeros((2, 1), np.int64), np.zeros(2, np.float32), np.zeros(2, np.int8), np.zeros(2, np.int8))
    plain = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=8, seed=1), SHAPE, np.uint8)
    fr = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=8, seed=1, frame_stack=4), SHAPE, np.uint8)
    dp, ds = prep.device_prev_stacks(), prep.device_stacks()
    with pytest.raises(B.BdrError, match="not a single-frame store"):
        plain.push_device_frames(dp, ROW, side[0], ds, ROW, *side[1:])
    raw = np.zeros(2 * ROW + 64, np.uint8)
    host = raw.ctypes.data + (-raw.ctypes.data) % 16                       # host rows, 16-byte aligned: refused for being host memory
    with pytest.raises(B.BdrError, match="device memory"):
        fr.push_device_frames(host, ROW, side[0], ds, ROW, *side[1:])
    with pytest.raises(B.BdrError, match="device memory"):
        fr.push_device_frames(dp, ROW, side[0], host, ROW, *side[1:])
    with pytest.raises(B.BdrError, match="strides must be >="):
        fr.push_device_frames(dp, ROW - 16, side[0], ds, ROW, *side[1:])
    with pytest.raises(B.BdrError, match="multiples of 16"):
        fr.push_device_frames(dp, ROW + 8, side[0], ds, ROW, *side[1:])
    with pytest.raises(B.BdrError, match="multiples of 16"):
        fr.push_device_frames(dp, ROW, side[0], ds, ROW + 4, *side[1:])
    big = torch.zeros(3 * ROW, dtype=torch.uint8, device="cuda:0")           # room for two rows behind an address that is 8 off
    torch.cuda.synchronize()
    with pytest.raises(B.BdrError, match="multiples of 16"):
        fr.push_device_frames(big.data_ptr() + 8, ROW, side[0], ds, ROW, *side[1:])
    with pytest.raises(B.BdrError, match="multiples of 16"):
        fr.push_device_frames(dp, ROW, side[0], big.data_ptr() + 8, ROW, *side[1:])
    with pytest.raises(B.BdrError, match="single-frame store"):
        fr.push_device(dp, ROW, side[0], ds, ROW, *side[1:])
    assert len(plain) == 0 and len(fr) == 0 and fr.head == 0 and fr.frames_used()[0] == 0
    fr.push_device_frames(dp, ROW, side[0], ds, ROW, *side[1:])               # and the buffer works
    assert len(fr) == 2
    plain.close(); fr.close(); prep.close()


# ------------------------------------------------------------------------------------------------ 6. the compiled Trainer loop
def test_compiled_trainer_with_device_observations_runs_over_the_single_frame_store(B):
    """bdr_trainer_train with bdr_env_vtable::obs_on_device over a single-frame store (its default push goes to
    bdr_replay_push_device_frames) against the same run over a plain ring: ring rows, index stream and trained parameters bit-equal."""
    from oracle import torch_ref as T
    out = []
    cap = 16
    for fs in (4, 0):
        env = B.AtariDeviceEnv(_Emulator(5, p_term=0.15), device_obs=True)
        rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=cap, seed=7, frame_stack=fs), SHAPE, np.uint8)
        a = _cnn(B, train=True)
        a.set_params(T.init_params(T.cnn_shapes(6), 3), "qnet"); a.set_params(T.init_params(T.cnn_shapes(6), 3), "qnet_tgt")
        a.set_explorer(B.EpsilonGreedy(final_step=40), seed=2)
        tr = B.NativeTrainer(B.TrainerConfig(max_opts=8, opt_interval=2, warmup_period=8))
        stats = tr.train(env, a, rb, SHAPE, np.uint8)
        a.sync()
        used = rb.frames_used()[0] if fs else None
        out.append((stats["env_steps"], stats["opt_steps"], stats["n_episodes"], rb.read_rows(0, cap), rb.sample_indices(8).tolist(),
                    a.get_params("qnet"), a.get_params("qnet_tgt"), used))
        a.close(); rb.close(); env.close()
    f, p = out
    assert f[:3] == p[:3] and f[1] == 8 and f[0] > cap          # the ring wrapped
    for x, y in zip(f[3], p[3]):
        assert (x.view(np.uint8) == y.view(np.uint8)).all()
    assert f[4] == p[4] and (f[5] == p[5]).all() and (f[6] == p[6]).all()
    print(f"frames_used, trainer loop, {f[0]} transitions, {f[2]} episodes: {f[7]}")
    assert f[7] < 3 * f[0]                                       # frames were shared: far fewer than the 8 per transition of unshared rows
