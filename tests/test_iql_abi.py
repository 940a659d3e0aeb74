"""The IQL entry points of the C ABI without a GPU: defaults equal border-candle-agent's (iql/config.rs:109-125, util/critic.rs:35-43,
util/actor.rs:44-55), and bdr_iql_create fails loudly when no device is visible."""
import ctypes as C

import pytest

from border_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_iql_symbols_are_exported(L):
    for name in ("bdr_iql_config_default", "bdr_iql_create", "bdr_iql_update_on_batch", "bdr_iql_probe", "bdr_iql_sample",
                 "bdr_iql_sample_device"):
        assert hasattr(L, name), name


def test_iql_config_default_is_the_reference_default(L):
    c = _lib.IqlConfigC()
    L.bdr_iql_config_default(C.byref(c))
    assert (c.gamma, c.tau_iql, c.inv_lambda, c.exp_adv_max) == (0.99, 0.7, 10.0, 100.0)
    assert (c.n_updates_per_opt, c.batch_size, c.adv_softmax, c.critic_loss) == (1, 1, 0, 0)
    assert (c.n_critics, c.critic_tau) == (2, 0.005)
    assert (c.min_log_std, c.max_log_std, c.action_limit, c.action_min, c.action_max) == (-20.0, 2.0, 0, -1.0, 1.0)
    for o, lr in ((c.opt_value, c.lr_value), (c.opt_actor, c.lr_actor), (c.opt_critic, c.lr_critic)):
        assert o.opt_kind == 0 and lr == 3e-4 and o.amsgrad == 0
    assert c.device == -1
    for m in (c.value, c.actor, c.critic):
        assert m.activation_out == 0


def test_python_config_maps_onto_the_struct(L):
    import border_amd as B
    cfg = B.IqlConfig(obs_dim=45, act_dim=24, adv_softmax=True, critic_loss="SmoothL1").lambda_(0.5)
    cfg.actor_config.action_limit = B.ActionLimit.Tanh(2.0)
    cfg.critic_config.opt_config = B.OptimizerConfig.AdamW(1e-3)
    c = cfg.to_c()
    assert c.inv_lambda == 2.0 and c.adv_softmax == 1 and c.critic_loss == 1
    assert c.action_limit == 1 and c.action_scale == 2.0
    assert c.opt_critic.opt_kind == 1 and c.lr_critic == 1e-3 and c.opt_critic.weight_decay == 0.01
    assert list(c.value.units[:c.value.n_units]) == [256, 256]


def test_iql_create_without_a_device_fails_loudly(L):
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    c = _lib.IqlConfigC()
    L.bdr_iql_config_default(C.byref(c))
    c.obs_dim, c.act_dim, c.device = 4, 2, 0
    for m in (c.value, c.actor, c.critic):
        m.n_units = 1; m.units[0] = 8
    h = C.c_void_p()
    assert L.bdr_iql_create(C.byref(c), C.byref(h)) == 2   # BDR_ERR_NO_DEVICE
    assert not h.value
