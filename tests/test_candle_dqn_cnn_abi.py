"""The C boundary of the candle DQN's AtariCnn form without a GPU: symbols, defaults, BDR_ERR_NO_DEVICE, and every refusal that is
decided before a device is looked for."""
import ctypes as C

import pytest

import border_amd as B
from border_amd import _lib


def _cfg(**kw):
    c = B.CandleDqnConfig(q_config=B.AtariCnnConfig(n_stack=4, out_dim=6), batch_size=4, device=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_symbols_and_defaults():
    L = _lib.lib()
    for name in ("bdr_candle_dqn_cnn_config_default", "bdr_candle_dqn_cnn_create", "bdr_candle_dqn_cnn_update_on_batch", "bdr_candle_dqn_probe"):
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS
    c, m = _lib.CandleDqnCnnConfigC(), _lib.CandleDqnConfigC()
    L.bdr_candle_dqn_cnn_config_default(C.byref(c)); L.bdr_candle_dqn_config_default(C.byref(m))
    assert (c.n_stack, c.out_dim, c.skip_linear, c.arithmetic) == (4, 0, 0, _lib.ARITHMETIC["f32_exact"])
    for f in ("lr", "soft_update_interval", "n_updates_per_opt", "batch_size", "discount_factor", "tau", "train", "double_dqn",
              "has_clip_reward", "has_clip_td_err", "critic_loss", "record_verbose_level", "device", "ckpt_format", "seed"):
        assert getattr(c, f) == getattr(m, f), f
    for f in ("opt_kind", "amsgrad", "beta1", "beta2", "weight_decay", "eps"):
        assert getattr(c.opt, f) == getattr(m.opt, f), f
    for f in ("kind", "eps_start", "eps_final", "final_step", "n_calls", "seed"):
        assert getattr(c.explorer, f) == getattr(m.explorer, f), f
    assert c.device == -1 and c.explorer.seed == 42
    # the Mlp form's struct keeps its size; the new one replaces obs_dim / n_actions / qnet by four ints
    assert C.sizeof(_lib.CandleDqnCnnConfigC) == C.sizeof(_lib.CandleDqnConfigC) - C.sizeof(_lib.MlpConfigC) - 8 + 16


def test_the_python_config_builds_the_cnn_form():
    c = _cfg()
    assert c.cnn and c.n_actions == 6 and c.obs_dim == 84 * 84 * 4
    assert isinstance(c.to_c(), _lib.CandleDqnCnnConfigC)
    m = B.CandleDqnConfig(obs_dim=4, n_actions=2)
    assert not m.cnn and isinstance(m.to_c(), _lib.CandleDqnConfigC)
    via_model = B.CandleDqnConfig(model_config=B.CandleDqnModelConfig(q_config=B.AtariCnnConfig(n_stack=2, out_dim=3)))
    assert via_model.cnn and via_model.to_c().n_stack == 2 and via_model.to_c().out_dim == 3


def test_no_device():
    """without a GPU a well-formed config gets BDR_ERR_NO_DEVICE; with one it builds"""
    if B.device_count() == 0:
        with pytest.raises(B.BdrError) as e:
            B.CandleDqn.build(_cfg())
        assert e.value.code == 2   # BDR_ERR_NO_DEVICE
    else:
        B.CandleDqn.build(_cfg()).close()


def test_refusals_decided_before_a_device_is_looked_for():
    """(they hold with and without a GPU: the checks run before the device is touched)"""
    def refused(match, **kw):
        with pytest.raises(B.BdrError, match=match) as e:
            B.CandleDqn.build(_cfg(**kw))
        assert e.value.code == 1, e.value   # BDR_ERR_INVALID
    refused("skip_linear", q_config=None, model_config=B.CandleDqnModelConfig(q_config=B.AtariCnnConfig(n_stack=4, out_dim=6, skip_linear=True)))
    refused("split-operand", arithmetic="bf16x3_6")
    refused("amsgrad", model_config=B.CandleDqnModelConfig(B.AtariCnnConfig(4, 6), B.OptimizerConfig.AdamW(1e-3, amsgrad=True)))
    for ns in (0, 9):
        refused("n_stack", model_config=B.CandleDqnModelConfig(q_config=B.AtariCnnConfig(n_stack=ns, out_dim=6)))
    refused("batch size", batch_size=0)
    with pytest.raises(B.BdrError, match="No device is given"):
        B.CandleDqn.build(_cfg(device=None))
