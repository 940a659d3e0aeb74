"""The candle DQN's AtariCnn form on the GPU (csrc/candle_dqn.hip, CandleDqnCnn) against tests/candle_dqn_cnn_restatement.py: goldens
and free runs over the committed cases, a ragged batch, the optimizer rule bit for bit (conv variables and the target's
track_element included), the out-of-range-action rule over the whole parameter set, the opt counters over a u8 ring, acting on host
and device rows, checkpoints, the launch count of one update and the refusals that need a device.

Bars: R.BAR = 4 x the largest float32-versus-float64 distance of the restatement over the committed cases, per quantity kind; the
device is measured against the float32 restatement and every figure is printed before it is asserted."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(__file__)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import candle_dqn_cnn_restatement as R  # noqa: E402
import candle_dqn_restatement as RM  # noqa: E402
import make_golden_candle_dqn_cnn as MG  # noqa: E402
import optimizer_inputs as OI  # noqa: E402

pytestmark = pytest.mark.gpu
ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01)
CASES = {c.name: c for c in R.CASES}


@pytest.fixture(scope="module")
def B():
    import border_amd
    if border_amd.device_count() == 0:
        pytest.fail("no MI355X visible: the HIP path must run on the GPU box")
    return border_amd


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _agent(B, spec, bsz, params, **kw):
    a = B.CandleDqn.build(spec.to_config(B, bsz, device=0, **kw))
    a.set_params(params[0], "qnet"); a.set_params(params[1], "qnet_tgt")
    return a


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the float32 restatement of a committed case, once per session: (quantities, per-update y)"""
    c = CASES[name]
    r, steps = R.run_case(c)
    return R.quantities(c, r, steps), [s["y"] for s in steps]


_DEVICE = {}


def _device(B, name):
    """the device's run of a committed case, once per session: the quantities of R.quantities, and y per update"""
    if name in _DEVICE:
        return _DEVICE[name]
    c = CASES[name]
    qnet, qnet_tgt, batches = R.case_inputs(c)
    a = _agent(B, c.spec, c.batch, (qnet, qnet_tgt))
    sl = R.var_slices(c.spec.n_stack, c.spec.n_actions)
    out, ys = {}, []
    for k, b in enumerate(batches):
        rec = a.update_on_batch(*b)
        out[f"loss/{k}"] = np.asarray([rec["loss"]])
        for key in R.PROBE_KEYS:
            out[f"{key}/{k}"] = a.probe(key, c.batch)
        ys.append(a.probe("y", c.batch))
        g = a.get_params("qnet", "grad")
        for v in R.VAR_NAMES:
            out[f"grad:{v}/{k}"] = g[sl[v]]
    out["qnet"], out["qnet_tgt"] = a.get_params("qnet"), a.get_params("qnet_tgt")
    assert a.n_opts == c.n_updates
    a.close()
    _DEVICE[name] = (out, ys)
    return _DEVICE[name]


# ---------------------------------------------------------------------------------------------------------- goldens, free runs
@pytest.mark.parametrize("name", sorted(CASES))
def test_goldens(B, name):
    """the committed results (loss, probes, gradient norms and sampled entries, sampled parameters) within the bars"""
    c = CASES[name]
    gold = np.load(MG.path_of(c))
    got, ys = _device(B, name)
    sl = R.var_slices(c.spec.n_stack, c.spec.n_actions)
    for k in range(c.n_updates):
        assert (ys[k] == gold[f"y/{k}"]).all(), (name, k, "y")
        for key in ("loss",) + R.PROBE_KEYS:
            d = R.distance(key, got[f"{key}/{k}"], gold[f"{key}/{k}"])
            print(name, k, key, d, "bar", R.BAR[key])
            assert d < R.BAR[key], (name, k, key, d)
        for v in R.VAR_NAMES:
            g = got[f"grad:{v}/{k}"]
            bar = R.BAR[f"grad:{v}"]
            norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
            dn = abs(norm - float(gold[f"grad_norm:{v}/{k}"])) / float(gold[f"grad_norm:{v}/{k}"])
            ds = np.abs(g[MG.sample_index(v, g.size)].astype(np.float64) - gold[f"grad_sample:{v}/{k}"]).max() / np.abs(g).max()
            print(name, k, "grad", v, "norm", dn, "sample", ds, "bar", bar)
            assert dn < bar and ds < bar, (name, k, v, dn, ds)
    for which in ("qnet", "qnet_tgt"):
        for v in R.VAR_NAMES:
            x = got[which][sl[v]]
            w = gold[f"{which}_sample:{v}"]
            d = np.abs(x[MG.sample_index(v, x.size)].astype(np.float64) - w).max()
            d = d if which == "qnet" else d / np.abs(got[which]).max()
            assert d < R.BAR[which], (name, which, v, d)


@pytest.mark.parametrize("name", sorted(CASES))
def test_free_run_against_the_restatement(B, name):
    """every compared quantity of every update, whole: probes, loss, all ten gradients, parameters and target parameters; no element
    is exempt"""
    got, ys = _device(B, name)
    want, wys = _reference(name)
    for k, (y, wy) in enumerate(zip(ys, wys)):
        assert (y == wy).all(), (name, k, "y")
    worst = {}
    for q in want:
        kind = R.kind_of(q)
        d = R.distance(kind, got[q], want[q])
        worst[kind] = max(worst.get(kind, 0.0), d)
    for kind, d in worst.items():
        print(name, kind, d, "bar", R.BAR[kind])
    for kind, d in worst.items():
        assert d < R.BAR[kind], (name, kind, d, R.BAR[kind])
    if CASES[name].tie:
        assert (ys[0] == 0).all()   # the first maximum of the exact tie


def test_a_terminal_row_takes_the_reward_bit_for_bit(B):
    got, _ = _device(B, R.CASES[0].name)
    _, _, batches = R.case_inputs(R.CASES[0])
    assert batches[0][4][0] == 1
    assert bits(got["tgt/0"][:1]) == bits(batches[0][3][:1])


# ---------------------------------------------------------------------------------------------------------- a ragged batch
RAGGED = R.CandleDqnCnnSpec(4, 6, lr=1e-7, adamw=ADAMW, double_dqn=True)


def test_a_ragged_batch_of_33(B):
    """conv M = 13 200 / 2 673 / 1 617 rows, no multiple of a 64-row tile: probes and loss (continuous across a ReLU flip) against
    the restatement, and two agents bit for bit"""
    params = RAGGED.init_params(77)
    batch = R.make_batch(RAGGED, 33, 78)
    ref = R.CandleDqnCnnRestatement(RAGGED, *params)
    assert RM.double_dqn_gap(ref, batch[2].astype(np.float32)) > 64 * R.F32_F64["pred"]
    rec = ref.update(*batch)
    a, b = _agent(B, RAGGED, 33, params), _agent(B, RAGGED, 33, params)
    ra, rb = a.update_on_batch(*batch), b.update_on_batch(*batch)
    assert ra == rb
    d = R.distance("loss", [ra["loss"]], [rec["loss"]])
    print("ragged loss", d)
    assert d < R.BAR["loss"]
    assert (a.probe("y", 33) == ref.probes["y"]).all()
    for key in R.PROBE_KEYS:
        d = R.distance(key, a.probe(key, 33), ref.probes[key])
        print("ragged", key, d, "bar", R.BAR[key])
        assert d < R.BAR[key], (key, d)
    for k in ("qnet", "qnet_tgt"):
        assert (bits(a.get_params(k)) == bits(b.get_params(k))).all(), k
    for role in ("grad", "exp_avg", "exp_avg_sq"):
        assert (bits(a.get_params("qnet", role)) == bits(b.get_params("qnet", role))).all(), role
    a.close(); b.close()


def test_a_batch_below_the_capacity_takes_the_same_step_bit_for_bit(B):
    """An agent built for 5 rows and one built for 2 take the same 2-row update: the weight-gradient partials are laid out for the
    capacity (conv_layout.hpp's conv_dw_plan) - conv2's and conv3's sit at other offsets in the two agents - but the chunks a batch
    fills follow the batch, 2, ceil(162 / 32) = 6 and ceil(98 / 32) = 4 in both, so k_cdqn_conv_reduce_adam sums the same sums:
    parameters, target parameters and the gradient arena equal byte for byte."""
    spec = R.CandleDqnCnnSpec(4, 6, lr=1e-4, tau=0.3, adamw=ADAMW, double_dqn=True)
    params = spec.init_params(91)
    assert (params[0] != params[1]).any()
    batch = R.make_batch(spec, 2, 92)
    got = []
    for cap in (5, 2):
        a = _agent(B, spec, cap, params)
        rec = a.update_on_batch(*batch)
        got.append((rec, a.get_params("qnet"), a.get_params("qnet_tgt"), a.get_params("qnet", "grad")))
        a.close()
    (ra, pa, ta, ga), (rb, pb, tb, gb) = got
    assert ra == rb
    assert pa.tobytes() == pb.tobytes() and ta.tobytes() == tb.tobytes() and ga.tobytes() == gb.tobytes()
    sl = R.var_slices(4, 6)
    for v in R.VAR_NAMES:   # the update ran: a gradient, a step and a soft update of every variable
        assert np.abs(ga[sl[v]]).max() > 0 and (pa[sl[v]] != params[0][sl[v]]).any() and (ta[sl[v]] != params[1][sl[v]]).any(), v


# ---------------------------------------------------------------------------------------------------------- the optimizer rule
@pytest.mark.parametrize("kind", ("AdamW", "Adam"))
def test_one_optimizer_step_and_the_soft_update_element_by_element(B, kind):
    """adam_element and track_element on the device's OWN gradient from crafted optimizer states (tests/optimizer_inputs.py's
    adam_f32 / track_f32), every variable - the conv ones go through k_cdqn_conv_reduce_adam: exp_avg and exp_avg_sq carry the
    restated bits; a parameter carries the bits of one of the three admitted roots (OI.SQRT_ULPS); the target those of track_f32"""
    o = OI.Opt("AdamW", 1e-2, 0.8, 0.9, 1e-3, 0.1) if kind == "AdamW" else OI.Opt("Adam", 3e-3)
    spec = R.CandleDqnCnnSpec(1, 3, lr=o.lr, tau=0.3, adamw=dict(beta1=o.b1, beta2=o.b2, eps=o.eps, wd=o.wd) if o.adamw else None)
    params = spec.init_params(10)
    a = _agent(B, spec, 3, params)
    rng = np.random.default_rng(11)
    m0 = (rng.standard_normal(spec.count()) * 1e-3).astype(np.float32)
    v0 = (rng.random(spec.count()) * 1e-5).astype(np.float32)
    a.set_params(m0, "qnet", "exp_avg"); a.set_params(v0, "qnet", "exp_avg_sq")
    p0, t0 = a.get_params("qnet"), a.get_params("qnet_tgt")
    a.update_on_batch(*R.make_batch(spec, 3, 4))
    g = a.get_params("qnet", "grad")
    sl = R.var_slices(1, 3)
    for v in R.VAR_NAMES:
        assert np.abs(g[sl[v]]).max() > 0, v
    s = OI.scalars_of(o, 1)
    forms = [OI.adam_f32(p0, g, m0, v0, None, s, u) for u in OI.SQRT_ULPS]
    m1, v1, p1, t1 = a.get_params("qnet", "exp_avg"), a.get_params("qnet", "exp_avg_sq"), a.get_params("qnet"), a.get_params("qnet_tgt")
    tau32, omt32 = OI.tau_scalars(spec.tau)
    want_t = OI.track_f32(p1, t0, tau32, omt32)
    for v in R.VAR_NAMES:
        assert (bits(m1[sl[v]]) == bits(forms[0][1][sl[v]])).all(), v
        assert (bits(v1[sl[v]]) == bits(forms[0][2][sl[v]])).all(), v
        ok = np.zeros(p1[sl[v]].shape, bool)
        for f in forms:
            ok |= bits(p1[sl[v]]) == bits(f[0][sl[v]])
        assert ok.all(), (v, int((~ok).sum()))
        assert not (bits(p1[sl[v]]) == bits(p0[sl[v]])).all(), v
        assert (bits(t1[sl[v]]) == bits(want_t[sl[v]])).all(), v
    a.close()


# ---------------------------------------------------------------------------------------------------------- action errors, counters
SMALL = R.CandleDqnCnnSpec(1, 3, adamw=ADAMW)


def _ring(B, spec, n, seed, per=False, obs_dtype=np.uint8, width=None):
    cfg = B.SimpleReplayBufferConfig(capacity=max(64, n), seed=seed)
    if per:
        cfg.per_config = B.PerConfig()
    rb = B.SimpleReplayBuffer(cfg, (width or spec.row_bytes,), obs_dtype, (1,), np.int64)
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, n, 70 + seed)
    w = width or spec.row_bytes
    rb.push(obs[:, :w].astype(obs_dtype), act.reshape(n, 1), nxt[:, :w].astype(obs_dtype), rew, term, trunc)
    return rb


def test_an_out_of_range_action_steps_nothing_and_the_next_clean_update_applies(B):
    spec = SMALL
    params = spec.init_params(7)
    a = _agent(B, spec, 4, params)
    obs, act, nxt, rew, term, trunc = R.make_batch(spec, 4, 3)
    a.update_on_batch(obs, act, nxt, rew, term, trunc)
    before = {k: a.get_params(k) for k in ("qnet", "qnet_tgt")}
    m0 = a.get_params("qnet", "exp_avg")
    rb = B.SimpleReplayBuffer(B.SimpleReplayBufferConfig(capacity=64, seed=1), (spec.row_bytes,), np.uint8, (1,), np.int64)
    rb.push(obs, np.full((4, 1), spec.n_actions, np.int64), nxt, rew, term, trunc)
    a.opt(rb)
    with pytest.raises(B.BdrError, match="action index outside"):
        a.sync()
    for k in before:   # conv variables included: the whole reference-layout vector
        assert (bits(a.get_params(k)) == bits(before[k])).all(), k
    assert (bits(a.get_params("qnet", "exp_avg")) == bits(m0)).all()
    bad = act.copy(); bad[2] = -1
    with pytest.raises(B.BdrError, match="action index outside"):
        a.update_on_batch(obs, bad, nxt, rew, term, trunc)
    for k in before:
        assert (bits(a.get_params(k)) == bits(before[k])).all(), k
    assert a.n_opts == 1
    twin = _agent(B, spec, 4, params)
    twin.update_on_batch(obs, act, nxt, rew, term, trunc)
    twin.update_on_batch(nxt, act, obs, rew, term, trunc)
    a.update_on_batch(nxt, act, obs, rew, term, trunc)
    for k in before:
        assert (bits(a.get_params(k)) == bits(twin.get_params(k))).all(), k
    assert not (bits(a.get_params("qnet")) == bits(before["qnet"])).all()
    assert a.n_opts == twin.n_opts == 2
    a.close(); twin.close(); rb.close()


def test_n_updates_per_opt_and_the_soft_update_interval_over_a_u8_ring(B):
    """n_updates_per_opt = 2, soft_update_interval = 2: the target changes on exactly the opts on which the restatement's does"""
    spec = R.CandleDqnCnnSpec(1, 3, adamw=ADAMW, n_updates_per_opt=2, soft_update_interval=2, tau=0.25)
    params = spec.init_params(8)
    a = _agent(B, spec, 2, params)
    ref = R.CandleDqnCnnRestatement(spec, *params)
    rb, rb2 = _ring(B, spec, 32, 5), _ring(B, spec, 32, 5)
    for o in range(4):
        t0, r0 = a.get_params("qnet_tgt"), ref.params("qnet_tgt")
        a.opt(rb)
        a.sync()
        bs = [rb2.batch(2) for _ in range(2)]
        ref.opt_([(x.obs, x.act.reshape(-1), x.next_obs, x.reward, x.is_terminated, x.is_truncated) for x in bs])
        moved = not (bits(a.get_params("qnet_tgt")) == bits(t0)).all()
        want = not (bits(ref.params("qnet_tgt")) == bits(r0)).all()
        assert moved == want == ((o + 1) % 2 == 0), (o, moved, want)
    assert a.n_opts == ref.n_opts == 4
    dt = RM.rel(a.get_params("qnet_tgt"), ref.params("qnet_tgt"))
    print("u8 ring, 8 updates: qnet_tgt", dt)
    assert dt < 1e-3   # (lr 1e-3 over 8 Adam steps: a sanity figure, the bars belong to the committed cases)
    a.close(); rb.close(); rb2.close()


# ---------------------------------------------------------------------------------------------------------- acting
ACT = R.CandleDqnCnnSpec(4, 6, adamw=ADAMW)


@pytest.mark.parametrize("n", (1, 9))
def test_acting_rows_equal_the_update_forward_bit_for_bit(B, n):
    """qnet_tgt = qnet, plain DQN: the update's probes are pred = Q(obs)[act] and q_next = max_j Q(next_obs)[j], so the acting call's
    Q rows must hold exactly those bits - host rows and device rows (dense and strided)"""
    p = ACT.init_params(21)[0]
    a = _agent(B, ACT, n, (p, p))
    obs, act, nxt, rew, term, trunc = R.make_batch(ACT, n, 22)
    q_o, q_n = a.qvalues(obs), a.qvalues(nxt)
    dense = torch.from_numpy(obs).cuda()
    wide = torch.zeros((n, ACT.row_bytes + 8), dtype=torch.uint8, device="cuda")
    wide[:, :ACT.row_bytes] = dense
    torch.cuda.synchronize()
    assert (bits(a.qvalues_device(dense.data_ptr(), n, ACT.row_bytes)) == bits(q_o)).all()
    assert (bits(a.qvalues_device(wide.data_ptr(), n, ACT.row_bytes + 8)) == bits(q_o)).all()
    assert (a.sample_greedy(obs) == q_o.argmax(1)).all()
    a.update_on_batch(obs, act, nxt, rew, term, trunc)
    assert (bits(a.probe("pred", n)) == bits(q_o[np.arange(n), act])).all()
    assert (bits(a.probe("q_next", n)) == bits(q_n.max(1))).all()
    assert (a.probe("y", n) == q_n.argmax(1)).all()
    ref = R.CandleDqnCnnRestatement(ACT, p, p)
    d = R.distance("pred", q_o, ref.qvalues(obs.astype(np.float32)))
    print("acting q", d)
    assert d < R.BAR["pred"]
    a.close()


@pytest.mark.parametrize("n", (1, 9))
def test_the_three_explorers_follow_the_restatements_small_rng(B, n):
    params = ACT.init_params(23)
    a = _agent(B, ACT, n, params, train=True, explorer=B.EpsilonGreedy(eps_start=1.0, eps_final=0.02, final_step=50))
    obs = R.make_batch(ACT, n, 24)[0]
    q = a.qvalues(obs)
    dev = torch.from_numpy(obs).cuda()
    torch.cuda.synchronize()
    ex = RM.CandleDqnExplorer("eps_greedy", 1.0, 0.02, 50, seed=42)
    for i in range(80):
        got = a.sample(obs) if i % 2 else a.sample_device(dev.data_ptr(), n, ACT.row_bytes)
        assert (got == ex.sample(q, True)).all(), i
    a.set_explorer(B.Softmax(), seed=7)
    ex = RM.CandleDqnExplorer("softmax", seed=7)
    for i in range(40):
        assert (a.sample(obs) == ex.sample(q, True)).all(), i
    a.eval()
    a.set_explorer(B.Softmax(), seed=9)
    ex = RM.CandleDqnExplorer(seed=9)
    got = np.array([a.sample(obs) for _ in range(400)])
    want = np.array([ex.sample(q, False) for _ in range(400)])
    assert (got == want).all()
    a.close()


# ---------------------------------------------------------------------------------------------------------- checkpoints
def _write_safetensors(path, tensors):
    import json
    import struct
    hdr, blob = {}, b""
    for name, arr in tensors:
        arr = np.ascontiguousarray(arr, np.float32)
        hdr[name] = {"dtype": "F32", "shape": list(arr.shape), "data_offsets": [len(blob), len(blob) + arr.nbytes]}
        blob += arr.tobytes()
    h = json.dumps(hdr).encode()
    h += b" " * (-len(h) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(h)) + h + blob)


def test_checkpoints_round_trip_and_a_file_in_reference_layout(B, tmp_path):
    spec = SMALL
    params = spec.init_params(16)
    a = _agent(B, spec, 2, params)
    a.update_on_batch(*R.make_batch(spec, 2, 1))
    d = str(tmp_path / "ck")
    assert [os.path.basename(p) for p in a.save_params(d)] == ["qnet.pt", "qnet_tgt.pt"] == sorted(os.listdir(d))
    b = _agent(B, spec, 2, spec.init_params(98))
    b.load_params(d)
    for k in ("qnet", "qnet_tgt"):
        assert (bits(a.get_params(k)) == bits(b.get_params(k))).all(), k
    d2 = str(tmp_path / "ck2")
    a.set_checkpoint_format("safetensors")
    assert [os.path.basename(p) for p in a.save_params(d2)] == ["qnet.safetensors", "qnet_tgt.safetensors"] == sorted(os.listdir(d2))
    c = _agent(B, spec, 2, spec.init_params(97))
    c.load_params(d2)                      # configured *.pt, only *.safetensors there
    for k in ("qnet", "qnet_tgt"):
        assert (bits(c.get_params(k)) == bits(a.get_params(k))).all(), k
    # a file written by the restatement in the reference's layout and names: the device gives the restatement's Q-values (a wrong
    # l1 column order would not)
    d3 = str(tmp_path / "ck3"); os.makedirs(d3)
    flat = spec.init_params(55)
    sl = R.var_slices(spec.n_stack, spec.n_actions)
    for stem, f in zip(("qnet", "qnet_tgt"), flat):
        ts = [(v, f[sl[v]].reshape(s)) for v, s in zip(R.VAR_NAMES, R.var_shapes(spec.n_stack, spec.n_actions))]
        _write_safetensors(os.path.join(d3, stem + ".pt"), ts[::-1])     # (any order in the file)
    b.load_params(d3)
    assert (bits(b.get_params("qnet")) == bits(flat[0])).all() and (bits(b.get_params("qnet_tgt")) == bits(flat[1])).all()
    obs = R.make_batch(spec, 3, 2)[0]
    ref = R.CandleDqnCnnRestatement(spec, *flat)
    dq = R.distance("pred", b.qvalues(obs), ref.qvalues(obs.astype(np.float32)))
    wrong = R.distance("pred", b.qvalues(obs), R.CandleDqnCnnRestatement(spec, *flat, hwc_flatten=True).qvalues(obs.astype(np.float32)))
    print("loaded file: q", dq, "against the (h, w, c) flatten", wrong)
    assert dq < R.BAR["pred"] < wrong
    _write_safetensors(os.path.join(d3, "qnet.pt"), [("c1.weight", np.zeros((32, 1, 8, 8)))])
    with pytest.raises(B.BdrError, match="missing"):
        b.load_params(d3)
    for x in (a, b, c):
        x.close()


# ---------------------------------------------------------------------------------------------------------- the launch schedule
@pytest.mark.parametrize("double", (False, True))
def test_one_update_takes_sixteen_launches_plus_the_gather(B, double):
    """from the profile brackets: conv1 / conv2 / conv3 forward (all passes per launch), l1 / l2 forward, k_cdqn_td, the two head
    input gradients, the grouped dW, the head's reduce + Adam, conv3 dW / dX, conv2 dW / dX, conv1 dW, the conv reduce + Adam"""
    spec = R.CandleDqnCnnSpec(4, 6, adamw=ADAMW, double_dqn=double)
    a = _agent(B, spec, 8, spec.init_params(1))
    rb = _ring(B, spec, 16, 1)
    a.opt(rb)
    a.profile_enable(True)
    a.opt(rb)
    a.sync()
    names = [k for k, _ in a.profile_read()]
    a.profile_enable(False)
    assert names == ["sample", "fwd_conv", "fwd_conv", "fwd_conv", "fwd", "fwd", "cdqn_td", "dx", "dx", "dw", "reduce_adam",
                     "conv3_dw", "conv3_dx", "conv2_dw", "conv2_dx", "conv1_dw", "conv_reduce_adam"], names
    assert len(names) - 1 == 16
    a.close(); rb.close()


# ---------------------------------------------------------------------------------------------------------- refusals with a device
def test_refusals_that_need_a_device(B):
    import ctypes as C
    spec = SMALL
    a = _agent(B, spec, 2, spec.init_params(1))
    f32 = _ring(B, spec, 8, 1, obs_dtype=np.float32)
    with pytest.raises(B.BdrError, match="not an f32 ring"):
        a.opt(f32)
    short = _ring(B, spec, 8, 1, width=84 * 84 - 4)
    with pytest.raises(B.BdrError, match="do not match"):
        a.opt(short)
    per = _ring(B, spec, 8, 1, per=True)
    with pytest.raises(B.BdrError, match=r"dqn/base\.rs:135-137"):
        a.opt(per)
    with pytest.raises(B.BdrError, match="fused acting kernel"):
        a.set_act_path("fused")
    L = B._lib.lib()
    with pytest.raises(B.BdrError, match="u8 frame stacks"):
        B._lib.check(L.bdr_agent_sample_raw(a.handle, None, 1, np.zeros(8, np.float32).ctypes.data_as(C.c_void_p), 0, 0, 0, None,
                                            np.zeros(1, np.int64).ctypes.data_as(C.c_void_p)))
    z = np.zeros(8, np.float32).ctypes.data_as(C.c_void_p)
    assert L.bdr_candle_dqn_update_on_batch(a.handle, 1, z, z, z, z, z, None, None) == 1 and b"u8" in L.bdr_last_error()
    assert a.n_opts == 0
    for x in (a, f32, short, per):
        x.close()
