"""The acting calls of the candle DQN CNN group (include/border_amd.h, csrc/candle_dqn_cnn_group.hpp) without a device: the symbols and
the null-argument refusals.  What needs members: tests/test_gpu_candle_dqn_cnn_group_act.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sample", "sample_members", "last_q")


def test_symbols():
    from border_amd import _lib
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    for n in NAMES:
        name = "bdr_candle_dqn_cnn_group_" + n
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS and re.search(r"BDR_API int32_t %s\((?:.|\n)*?dqn/base\.rs" % name, text), n


def test_null_arguments_are_refused():
    from border_amd import _lib
    L = _lib.lib()
    g = C.cast(C.create_string_buffer(8), C.c_void_p)   # (never read: the null check comes first)
    one, ix, out = (C.c_void_p * 1)(None), (C.c_uint32 * 1)(0), (C.c_float * 8)()
    calls = (
        lambda: L.bdr_candle_dqn_cnn_group_sample(None, 1, one, one),
        lambda: L.bdr_candle_dqn_cnn_group_sample(g, 1, None, one),
        lambda: L.bdr_candle_dqn_cnn_group_sample(g, 1, one, None),
        lambda: L.bdr_candle_dqn_cnn_group_sample_members(None, ix, 1, 1, one, one),
        lambda: L.bdr_candle_dqn_cnn_group_sample_members(g, None, 1, 1, one, one),
        lambda: L.bdr_candle_dqn_cnn_group_sample_members(g, ix, 1, 1, None, one),
        lambda: L.bdr_candle_dqn_cnn_group_sample_members(g, ix, 1, 1, one, None),
        lambda: L.bdr_candle_dqn_cnn_group_last_q(None, 0, out, 8),
        lambda: L.bdr_candle_dqn_cnn_group_last_q(g, 0, None, 8),
    )
    for i, call in enumerate(calls):
        assert call() == 1 and b"null" in L.bdr_last_error(), i   # BDR_ERR_INVALID
