"""The C ABI of the candle DQN CNN group (include/border_amd.h, csrc/candle_dqn_cnn_group.hpp) without a device: the symbols, the form id,
the null-argument refusals, and bdr_candle_dqn_cnn_group_create of members on a machine without a GPU (BDR_ERR_NO_DEVICE from building
the members).  What needs members: tests/test_gpu_candle_dqn_cnn_group.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("create", "destroy", "size", "member", "info", "opt", "opt_with_record", "sync")


def test_symbols_and_the_form_id():
    from border_amd import _lib
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    for n in NAMES:
        assert hasattr(L, "bdr_candle_dqn_cnn_group_" + n) and re.search(r"BDR_API int32_t bdr_candle_dqn_cnn_group_%s\(.*dqn/base\.rs" % n, text), n
    assert int(re.search(r"#define BDR_GROUP_FORM_CANDLE_DQN_CNN_LAYERS (\d+)", text).group(1)) == _lib.GROUP_FORM_CANDLE_DQN_CNN_LAYERS == 7
    import border_amd
    assert border_amd.CandleDqnCnnGroup._PREFIX == "bdr_candle_dqn_cnn_group"


def test_null_arguments_are_refused():
    from border_amd import _lib
    L = _lib.lib()
    g, a, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
    info = _lib.GroupInfoC()
    one = (C.c_void_p * 1)(None)
    out, cnt = (C.c_float * 8)(), (C.c_int32 * 1)()
    calls = (
        lambda: L.bdr_candle_dqn_cnn_group_create(None, 1, C.byref(g)),
        lambda: L.bdr_candle_dqn_cnn_group_create(one, 1, None),
        lambda: L.bdr_candle_dqn_cnn_group_size(None, C.byref(n)),
        lambda: L.bdr_candle_dqn_cnn_group_member(None, 0, C.byref(a)),
        lambda: L.bdr_candle_dqn_cnn_group_info(None, C.byref(info)),
        lambda: L.bdr_candle_dqn_cnn_group_opt(None, one),
        lambda: L.bdr_candle_dqn_cnn_group_opt_with_record(None, one, out, 8, cnt),
        lambda: L.bdr_candle_dqn_cnn_group_sync(None),
    )
    for i, call in enumerate(calls):
        assert call() == 1 and b"null" in L.bdr_last_error(), i   # BDR_ERR_INVALID
    assert L.bdr_candle_dqn_cnn_group_destroy(None) == 0
    assert L.bdr_candle_dqn_cnn_group_create(one, 0, C.byref(g)) == 1 and b"1 .. 65535 members" in L.bdr_last_error()
    assert L.bdr_candle_dqn_cnn_group_create(one, 1, C.byref(g)) == 1 and b"member 0: null agent" in L.bdr_last_error()


def test_create_without_a_device_is_no_device():
    import border_amd as B
    cfg = B.CandleDqnConfig(q_config=B.AtariCnnConfig(n_stack=1, out_dim=3), batch_size=2, device=0)
    if B.device_count() > 0:
        g = B.CandleDqnCnnGroup.build([cfg])      # with one, a group of one exists and says what it is
        assert g.form == "candle_dqn_cnn_layers" and g.launches_per_round == 17 and len(g) == 1
        g.close()
        return
    with pytest.raises(B.BdrError) as e:
        B.CandleDqnCnnGroup.build([cfg, cfg])
    assert e.value.code == 2   # BDR_ERR_NO_DEVICE
