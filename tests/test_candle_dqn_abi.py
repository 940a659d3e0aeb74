"""The candle DQN entry points of the C ABI without a GPU: the symbols are exported by the cross-compiled library, the defaults equal
border-candle-agent's (dqn/config.rs:75-102, dqn/model.rs, dqn/explorer.rs, dqn/base.rs:274), the Python config maps onto the struct,
bdr_candle_dqn_create fails loudly when no device is visible, and what the agent cannot run is refused with the reason before any
device is looked for."""
import ctypes as C

import pytest

from border_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_candle_dqn_symbols_are_exported(L):
    for name in ("bdr_candle_dqn_config_default", "bdr_candle_dqn_create", "bdr_candle_dqn_update_on_batch", "bdr_candle_dqn_probe"):
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name


def test_candle_dqn_config_default_is_the_reference_default(L):
    c = _lib.CandleDqnConfigC()
    L.bdr_candle_dqn_config_default(C.byref(c))
    assert (c.soft_update_interval, c.n_updates_per_opt, c.batch_size) == (1, 1, 1)
    assert (c.discount_factor, c.tau, c.train) == (0.99, 0.005, 0)
    assert (c.has_clip_reward, c.double_dqn, c.has_clip_td_err, c.device) == (0, 0, 0, -1)
    assert (c.critic_loss, c.record_verbose_level) == (0, 0)                                   # CriticLoss::Mse
    e = c.explorer
    assert (e.kind, e.eps_start, e.eps_final, e.final_step, e.n_calls) == (0, 1.0, 0.02, 100000, 0)   # DqnExplorer::Softmax
    assert e.seed == 42                                                                        # SmallRng::seed_from_u64(42)
    # DqnModelConfig: OptimizerConfig::default() = AdamW with candle's ParamsAdamW defaults
    assert (c.opt.opt_kind, c.opt.amsgrad, c.opt.beta1, c.opt.beta2, c.opt.weight_decay, c.opt.eps, c.lr) == (1, 0, 0.9, 0.999, 0.01, 1e-8, 1e-3)
    assert c.qnet.activation_out == 0 and c.ckpt_format == 0


def test_python_config_maps_onto_the_struct(L):
    import border_amd as B
    cfg = B.CandleDqnConfig(obs_dim=4, n_actions=2, soft_update_interval=5, n_updates_per_opt=2, batch_size=64, discount_factor=0.98, tau=0.01,
                            train=True, double_dqn=True, clip_reward=1.0, clip_td_err=(-1.0, 1.0), critic_loss="SmoothL1", record_verbose_level=2,
                            explorer=B.EpsilonGreedy(n_opts=3, eps_start=0.9, eps_final=0.1, final_step=1000), explorer_seed=7, seed=11,
                            ckpt_format="safetensors",
                            model_config=B.CandleDqnModelConfig(B.CandleMlpConfig((64, 32), "ReLU"), B.OptimizerConfig.Adam(3e-4)))
    c = cfg.to_c()
    assert (c.obs_dim, c.n_actions, c.soft_update_interval, c.n_updates_per_opt, c.batch_size) == (4, 2, 5, 2, 64)
    assert (c.discount_factor, c.tau, c.train, c.double_dqn, c.critic_loss, c.record_verbose_level) == (0.98, 0.01, 1, 1, 1, 2)
    assert (c.has_clip_reward, c.clip_reward, c.has_clip_td_err, c.clip_td_err_min, c.clip_td_err_max) == (1, 1.0, 1, -1.0, 1.0)
    e = c.explorer
    assert (e.kind, e.eps_start, e.eps_final, e.final_step, e.n_calls, e.seed) == (1, 0.9, 0.1, 1000, 3, 7)
    assert list(c.qnet.units[:c.qnet.n_units]) == [64, 32] and c.qnet.activation_out == 1
    assert (c.opt.opt_kind, c.lr, c.seed, c.ckpt_format, c.device) == (0, 3e-4, 11, 1, -1)
    d = B.CandleDqnConfig(obs_dim=4, n_actions=2).to_c()
    assert (d.explorer.kind, d.explorer.seed, d.opt.opt_kind, d.opt.weight_decay, d.lr) == (0, 42, 1, 0.01, 1e-3)


def _small(L):
    c = _lib.CandleDqnConfigC()
    L.bdr_candle_dqn_config_default(C.byref(c))
    c.obs_dim, c.n_actions, c.device, c.batch_size = 4, 2, 0, 8
    c.qnet.n_units = 2; c.qnet.units[0] = 8; c.qnet.units[1] = 8
    return c


def test_candle_dqn_create_without_a_device_fails_loudly(L):
    c = _small(L)
    h = C.c_void_p()
    st = L.bdr_candle_dqn_create(C.byref(c), C.byref(h))
    if _lib.device_count() == 0:
        assert st == 2 and not h.value   # BDR_ERR_NO_DEVICE
    else:
        assert st == 0 and h.value
        L.bdr_agent_destroy(h)
    c.device = -1
    h = C.c_void_p()
    assert L.bdr_candle_dqn_create(C.byref(c), C.byref(h)) == 1 and b"No device is given for DQN agent" in L.bdr_last_error() and not h.value


def _refused(L, c, reason):
    h = C.c_void_p()
    assert L.bdr_candle_dqn_create(C.byref(c), C.byref(h)) == 1, reason   # BDR_ERR_INVALID, GPU or not
    assert reason in L.bdr_last_error(), L.bdr_last_error()
    assert not h.value


def test_candle_dqn_create_refuses_before_looking_for_a_device(L):
    c = _small(L); c.critic_loss = 7
    _refused(L, c, b"unknown critic loss")
    c = _small(L); c.opt.opt_kind = 5
    _refused(L, c, b"unknown optimizer")
    c = _small(L); c.opt.opt_kind = 1; c.opt.amsgrad = 1
    _refused(L, c, b"amsgrad")                                # candle's AdamW has no amsgrad
    c = _small(L); c.n_actions = 0
    _refused(L, c, b"n_actions")
    c = _small(L); c.qnet.units[1] = 4097
    _refused(L, c, b"bad layer width")
    c = _small(L); c.qnet.activation_out = 2
    _refused(L, c, b"activation_out")
    c = _small(L); c.explorer.kind = 4
    _refused(L, c, b"unknown explorer")
    c = _small(L); c.explorer.kind = 1; c.explorer.final_step = 0
    _refused(L, c, b"final_step")
    c = _small(L); c.soft_update_interval = 0
    _refused(L, c, b"intervals")
    assert L.bdr_candle_dqn_update_on_batch(None, 1, None, None, None, None, None, None, None) == 1
    assert L.bdr_candle_dqn_probe(None, 0, None, 1) == 1
