"""The BC entry points of the C ABI without a GPU: defaults equal border-candle-agent's (bc/config.rs:66-75, bc/model.rs:33-43), the
Python config maps onto the struct, bdr_bc_create fails loudly when no device is visible, and what it refuses it refuses before it
looks for a device."""
import ctypes as C

import pytest

from border_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_bc_symbols_are_exported(L):
    for name in ("bdr_bc_config_default", "bdr_bc_create", "bdr_bc_update_on_batch", "bdr_bc_probe", "bdr_bc_sample",
                 "bdr_bc_sample_device"):
        assert hasattr(L, name), name


def test_bc_config_default_is_the_reference_default(L):
    c = _lib.BcConfigC()
    L.bdr_bc_config_default(C.byref(c))
    assert (c.batch_size, c.action_type, c.device, c.record_verbose_level) == (1, 0, -1, 0)   # Discrete, no device
    assert c.policy.activation_out == 0 and c.policy.n_units == 0
    # OptimizerConfig::default(): AdamW with candle's ParamsAdamW defaults
    assert (c.opt.opt_kind, c.lr, c.opt.beta1, c.opt.beta2, c.opt.eps, c.opt.weight_decay, c.opt.amsgrad) == (1, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0)
    assert (c.kernel_form, c.head_rows) == (0, 0)


def test_python_config_maps_onto_the_struct(L):
    import border_amd as B
    d = B.BcConfig()
    assert (d.batch_size, d.action_type, d.device, d.record_verbose_level) == (1, B.BcActionType.Discrete, None, 0)
    cfg = B.BcConfig(obs_dim=45, act_dim=24, batch_size=256, action_type=B.BcActionType.Continuous, seed=7, kernel_form="fused", head_rows=8,
                     policy_model_config=B.BcModelConfig(B.CandleMlpConfig((256, 128), "Tanh"), B.OptimizerConfig.Adam(3e-4)))
    c = cfg.to_c()
    assert (c.obs_dim, c.act_dim, c.batch_size, c.action_type, c.device, c.seed) == (45, 24, 256, 1, -1, 7)
    assert list(c.policy.units[:c.policy.n_units]) == [256, 128] and c.policy.activation_out == 2
    assert c.opt.opt_kind == 0 and c.lr == 3e-4
    assert (c.kernel_form, c.head_rows) == (2, 8)
    cfg.policy_model_config = B.BcModelConfig(B.CandleMlpConfig((64,), "Sigmoid"), B.OptimizerConfig.AdamW(1e-3, wd=0.05))
    c = cfg.to_c()
    assert c.policy.activation_out == 3 and c.opt.opt_kind == 1 and c.opt.weight_decay == 0.05


def _small(L):
    c = _lib.BcConfigC()
    L.bdr_bc_config_default(C.byref(c))
    c.obs_dim, c.act_dim, c.device, c.batch_size, c.action_type = 4, 2, 0, 8, 1
    c.policy.n_units = 1; c.policy.units[0] = 8
    return c


def test_bc_create_without_a_device_fails_loudly(L):
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    for act_out in range(4):            # all four output activations pass the checks
        for action_type in (0, 1):      # create works for Discrete too
            c = _small(L)
            c.policy.activation_out, c.action_type = act_out, action_type
            h = C.c_void_p()
            assert L.bdr_bc_create(C.byref(c), C.byref(h)) == 2   # BDR_ERR_NO_DEVICE
            assert not h.value
    c = _small(L)
    c.device = -1
    h = C.c_void_p()
    assert L.bdr_bc_create(C.byref(c), C.byref(h)) == 1 and b"No device is given" in L.bdr_last_error()


@pytest.mark.parametrize("field,value,msg", [
    ("activation_out", 4, b"activation_out"), ("activation_out", -1, b"activation_out"), ("action_type", 2, b"action type"),
    ("kernel_form", 4, b"kernel form"), ("head_rows", 12, b"head_rows"),
])
def test_bc_create_refuses_before_it_looks_for_a_device(L, field, value, msg):
    c = _small(L)
    setattr(c.policy if field == "activation_out" else c, field, value)
    h = C.c_void_p()
    assert L.bdr_bc_create(C.byref(c), C.byref(h)) == 1   # BDR_ERR_INVALID, GPU or not
    assert msg in L.bdr_last_error()
    assert not h.value


def test_a_forced_fused_head_is_refused_where_it_does_not_apply(L):
    for act_dim, n_units, width in ((65, 1, 8), (2, 0, 0), (2, 1, 1024)):
        c = _small(L)
        c.act_dim, c.kernel_form, c.policy.n_units = act_dim, 2, n_units
        if n_units:
            c.policy.units[0] = width
        h = C.c_void_p()
        assert L.bdr_bc_create(C.byref(c), C.byref(h)) == 1
        assert b"BDR_BC_KERNEL_GENERAL" in L.bdr_last_error()
    for act_dim, n_units in ((65, 1), (2, 0)):      # the MFMA head has no LDS plan to exceed
        c = _small(L)
        c.act_dim, c.kernel_form, c.policy.n_units = act_dim, 3, n_units
        h = C.c_void_p()
        assert L.bdr_bc_create(C.byref(c), C.byref(h)) == 1
        assert b"BDR_BC_KERNEL_GENERAL" in L.bdr_last_error()
