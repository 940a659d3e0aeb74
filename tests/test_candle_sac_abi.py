"""The candle SAC entry points of the C ABI without a GPU: defaults equal border-candle-agent's (sac/config.rs:82-93,
util/critic.rs:35-43, util/actor.rs:44-55), the Python config maps onto the struct, bdr_candle_sac_create fails loudly when no
device is visible, and what the reference cannot run is refused with the reason before any device is looked for."""
import ctypes as C

import pytest

from border_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_candle_sac_symbols_are_exported(L):
    for name in ("bdr_candle_sac_config_default", "bdr_candle_sac_create", "bdr_candle_sac_update_on_batch", "bdr_candle_sac_probe",
                 "bdr_candle_sac_sample", "bdr_candle_sac_sample_device"):
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name


def test_candle_sac_config_default_is_the_reference_default(L):
    c = _lib.CandleSacConfigC()
    L.bdr_candle_sac_config_default(C.byref(c))
    assert c.gamma == 0.99 and (c.ent_coef_mode, c.ent_coef_alpha) == (0, 1.0)          # EntCoefMode::Fix(1.0)
    assert (c.n_updates_per_opt, c.batch_size, c.critic_loss, c.train) == (1, 1, 0, 0)
    assert (c.n_critics, c.critic_tau) == (2, 0.005)
    assert (c.min_log_std, c.max_log_std, c.action_limit, c.action_min, c.action_max) == (-20.0, 2.0, 0, -1.0, 1.0)
    for o, lr in ((c.opt_actor, c.lr_actor), (c.opt_critic, c.lr_critic)):
        assert o.opt_kind == 0 and lr == 3e-4 and o.amsgrad == 0
    assert c.device == -1 and c.actor_kind == 0
    for m in (c.actor, c.critic):
        assert m.activation_out == 0


def test_python_config_maps_onto_the_struct(L):
    import border_amd as B
    cfg = B.CandleSacConfig(obs_dim=3, act_dim=1, critic_loss="SmoothL1", n_updates_per_opt=3, batch_size=128, gamma=0.98,
                            ent_coef_mode=B.EntCoefMode.Auto(-1.0, 1e-3))
    cfg.actor_config = B.GaussianActorConfig(B.CandleMlpConfig((64, 32)), B.OptimizerConfig.Adam(1e-4), -5.0, 1.0, B.ActionLimit.Tanh(2.0), kind="Mlp2")
    cfg.critic_config = B.MultiCriticConfig(3, B.CandleMlpConfig((64, 32), "ReLU"), B.OptimizerConfig.AdamW(1e-3), 0.01)
    c = cfg.to_c()
    assert (c.ent_coef_mode, c.target_entropy, c.ent_coef_lr) == (1, -1.0, 1e-3) and c.gamma == 0.98 and c.critic_loss == 1
    assert c.actor_kind == 1 and c.action_limit == 1 and c.action_scale == 2.0 and (c.min_log_std, c.max_log_std) == (-5.0, 1.0)
    assert c.n_critics == 3 and c.critic_tau == 0.01 and c.lr_actor == 1e-4
    assert c.opt_critic.opt_kind == 1 and c.lr_critic == 1e-3 and c.opt_critic.weight_decay == 0.01
    assert list(c.critic.units[:c.critic.n_units]) == [64, 32] and c.critic.activation_out == 1
    assert list(c.actor.units[:c.actor.n_units]) == [64, 32]
    assert (c.n_updates_per_opt, c.batch_size, c.train, c.device) == (3, 128, 0, -1)
    d = B.CandleSacConfig(obs_dim=3, act_dim=1, ent_coef_mode=B.EntCoefMode.Fix(0.2)).to_c()
    assert (d.ent_coef_mode, d.ent_coef_alpha, d.actor_kind) == (0, 0.2, 0)
    assert B.GaussianActorConfig().kind == "Mlp3"      # IQL and AWAC build Mlp3 whatever it says


def _small(L):
    c = _lib.CandleSacConfigC()
    L.bdr_candle_sac_config_default(C.byref(c))
    c.obs_dim, c.act_dim, c.device, c.batch_size, c.actor_kind = 4, 2, 0, 8, 1
    for m in (c.actor, c.critic):
        m.n_units = 2; m.units[0] = 8; m.units[1] = 8
    return c


def test_candle_sac_create_without_a_device_fails_loudly(L):
    c = _small(L)
    h = C.c_void_p()
    st = L.bdr_candle_sac_create(C.byref(c), C.byref(h))
    if _lib.device_count() == 0:
        assert st == 2 and not h.value   # BDR_ERR_NO_DEVICE
    else:
        assert st == 0 and h.value
        L.bdr_agent_destroy(h)
    c.device = -1
    h = C.c_void_p()
    assert L.bdr_candle_sac_create(C.byref(c), C.byref(h)) == 1 and b"No device is given" in L.bdr_last_error() and not h.value


def _refused(L, c, reason):
    h = C.c_void_p()
    assert L.bdr_candle_sac_create(C.byref(c), C.byref(h)) == 1, reason   # BDR_ERR_INVALID, GPU or not
    assert reason in L.bdr_last_error(), L.bdr_last_error()
    assert not h.value


def test_candle_sac_create_refuses_what_the_reference_cannot_run_before_looking_for_a_device(L):
    c = _small(L); c.batch_size = 1
    _refused(L, c, b"at least 2 rows")                       # the squeeze at sac/base.rs:83
    c = _small(L); c.actor.n_units = 1
    _refused(L, c, b"at least 2 layers")                     # mlp.rs:14-24: 0..=n_layers-2 underflows
    c.actor_kind = 0                                         # ... while Mlp3 runs with one hidden layer (refused below only for the device)
    c = _small(L); c.actor_kind = 7
    _refused(L, c, b"unknown actor_kind")
    for which in ("opt_actor", "opt_critic"):
        c = _small(L)
        getattr(c, which).opt_kind = 1; getattr(c, which).amsgrad = 1
        _refused(L, c, b"amsgrad")                           # candle's AdamW has no amsgrad
    c = _small(L); c.ent_coef_mode = 5
    _refused(L, c, b"unknown ent_coef_mode")
