"""The split-operand arithmetic of the candle DQN's AtariCnn form at the C boundary, without a GPU: it is set on a built agent
(bdr_candle_dqn_cnn_set_arithmetic), so what can be seen here is the symbols and the refusals decided before an agent is looked at."""
import pytest

import border_amd as B
from border_amd import _lib


def test_the_new_symbols():
    for name in ("bdr_candle_dqn_cnn_set_arithmetic", "bdr_candle_dqn_cnn_keep_layers"):
        assert hasattr(_lib.lib(), name) and name in _lib.ABI_SYMBOLS


def test_a_null_agent_is_refused():
    assert _lib.lib().bdr_candle_dqn_cnn_set_arithmetic(None, _lib.ARITHMETIC["bf16x3_6"]) == 1
    assert _lib.lib().bdr_candle_dqn_cnn_keep_layers(None, 1) == 1


def test_the_constructors_refusal_names_the_switch():
    cfg = B.CandleDqnConfig(q_config=B.AtariCnnConfig(n_stack=4, out_dim=6), batch_size=4, device=0, arithmetic="bf16x3_6")
    with pytest.raises(B.BdrError, match="bdr_candle_dqn_cnn_set_arithmetic") as e:
        B.CandleDqn.build(cfg)
    assert e.value.code == 1
