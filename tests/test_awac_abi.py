"""The AWAC entry points of the C ABI without a GPU: defaults equal border-candle-agent's (awac/config.rs:120-141, util/critic.rs:35-43,
util/actor.rs:44-55), the Python config maps onto the struct, and bdr_awac_create fails loudly when no device is visible."""
import ctypes as C

import pytest

from border_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_awac_symbols_are_exported(L):
    for name in ("bdr_awac_config_default", "bdr_awac_create", "bdr_awac_update_on_batch", "bdr_awac_probe", "bdr_awac_sample",
                 "bdr_awac_sample_device"):
        assert hasattr(L, name), name


def test_awac_config_default_is_the_reference_default(L):
    c = _lib.AwacConfigC()
    L.bdr_awac_config_default(C.byref(c))
    assert (c.gamma, c.inv_lambda, c.exp_adv_max) == (0.99, 10.0, 100.0)
    assert (c.n_updates_per_opt, c.batch_size, c.adv_softmax, c.critic_loss, c.train) == (1, 1, 0, 0, 0)
    assert (c.n_critics, c.critic_tau) == (2, 0.005)
    assert (c.min_log_std, c.max_log_std, c.action_limit, c.action_min, c.action_max) == (-20.0, 2.0, 0, -1.0, 1.0)
    for o, lr in ((c.opt_actor, c.lr_actor), (c.opt_critic, c.lr_critic)):
        assert o.opt_kind == 0 and lr == 3e-4 and o.amsgrad == 0
    assert c.device == -1
    for m in (c.actor, c.critic):
        assert m.activation_out == 0


def test_python_config_maps_onto_the_struct(L):
    import border_amd as B
    cfg = B.AwacConfig(obs_dim=45, act_dim=24, adv_softmax=True, critic_loss="SmoothL1", n_updates_per_opt=3, batch_size=256).lambda_(0.5)
    cfg.actor_config.action_limit = B.ActionLimit.Tanh(2.0)
    cfg.actor_config.min_log_std = -5.0
    cfg.critic_config = B.MultiCriticConfig(3, B.CandleMlpConfig((64, 32), "ReLU"), B.OptimizerConfig.AdamW(1e-3), 0.01)
    c = cfg.to_c()
    assert c.inv_lambda == 2.0 and c.adv_softmax == 1 and c.critic_loss == 1
    assert c.action_limit == 1 and c.action_scale == 2.0 and c.min_log_std == -5.0
    assert c.n_critics == 3 and c.critic_tau == 0.01
    assert c.opt_critic.opt_kind == 1 and c.lr_critic == 1e-3 and c.opt_critic.weight_decay == 0.01
    assert list(c.critic.units[:c.critic.n_units]) == [64, 32] and c.critic.activation_out == 1
    assert list(c.actor.units[:c.actor.n_units]) == [256, 256]
    assert (c.n_updates_per_opt, c.batch_size, c.train, c.device) == (3, 256, 0, -1)


def _small(L):
    c = _lib.AwacConfigC()
    L.bdr_awac_config_default(C.byref(c))
    c.obs_dim, c.act_dim, c.device, c.batch_size = 4, 2, 0, 8
    for m in (c.actor, c.critic):
        m.n_units = 1; m.units[0] = 8
    return c


def test_awac_create_without_a_device_fails_loudly(L):
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    c = _small(L)
    h = C.c_void_p()
    assert L.bdr_awac_create(C.byref(c), C.byref(h)) == 2   # BDR_ERR_NO_DEVICE
    assert not h.value


def test_awac_create_rejects_a_one_row_batch_before_looking_for_a_device(L):
    """the reference cannot run B = 1 (include/border_amd.h, bdr_awac_config): BDR_ERR_INVALID with the reason, GPU or not"""
    c = _small(L)
    c.batch_size = 1
    h = C.c_void_p()
    assert L.bdr_awac_create(C.byref(c), C.byref(h)) == 1   # BDR_ERR_INVALID
    assert b"at least 2 rows" in L.bdr_last_error()
    assert not h.value
