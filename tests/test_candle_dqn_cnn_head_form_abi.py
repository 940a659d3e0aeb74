"""The head form of the candle DQN's AtariCnn form at the C boundary, without a GPU: it is set on a built agent
(bdr_candle_dqn_cnn_set_head_form), so what can be seen here is the symbol, its values and the refusals decided before an agent is looked at."""
import border_amd as B
from border_amd import _lib


def test_the_new_symbol_and_its_values():
    assert hasattr(_lib.lib(), "bdr_candle_dqn_cnn_set_head_form") and "bdr_candle_dqn_cnn_set_head_form" in _lib.ABI_SYMBOLS
    assert _lib.HEAD_FORM == {"layers": 0, "splitk": 1}
    assert callable(B.CandleDqn.set_head_form)


def test_a_null_agent_is_refused_whatever_the_value():
    for value in (_lib.HEAD_FORM["layers"], _lib.HEAD_FORM["splitk"], 7):
        assert _lib.lib().bdr_candle_dqn_cnn_set_head_form(None, value) == 1
        assert b"null argument" in _lib.lib().bdr_last_error()
