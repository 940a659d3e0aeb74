"""The candle DQN group's entry points of the C ABI without a GPU: the symbols are exported and declared, NULL arguments are
BDR_ERR_INVALID, and everything bdr_candle_dqn_group_create refuses before a device is looked for - a member list that is empty or too
long, a NULL member - is refused without one.  Without a device no member can exist: bdr_candle_dqn_create fails with
BDR_ERR_NO_DEVICE, so no group can either."""
import ctypes as C
import os
import re

import pytest

from border_amd import _lib, build

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "border_amd.h")
NEW = tuple("bdr_candle_dqn_group_" + n for n in ("create", "destroy", "size", "member", "info", "opt", "opt_with_scalars", "sync", "sample", "sample_members",
                                                  "last_q", "push", "push_max_rows"))
NEW_VOID = tuple("bdr_candle_dqn_group_" + n for n in ("trainer_ops_default", "eval_ops_default", "trainer_post_default"))
INVALID = 1   # BDR_ERR_INVALID


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_the_new_symbols_are_exported_and_declared(L):
    text = open(HEADER).read()
    for name in NEW + NEW_VOID:
        assert hasattr(L, name), name
        assert re.search(r"BDR_API %s %s\(" % ("void" if name in NEW_VOID else "int32_t", name), text), name
        assert name in _lib.ABI_SYMBOLS, name
    assert int(re.search(r"#define BDR_GROUP_FORM_CANDLE_DQN_LAYERS (\d+)", text).group(1)) == _lib.GROUP_FORM_CANDLE_DQN_LAYERS == 6
    import border_amd
    assert border_amd.group.GROUP_FORMS[6] == "candle_dqn_layers" and issubclass(border_amd.CandleDqnGroup, border_amd.group._GroupBase)


def test_null_arguments_are_invalid(L):
    g, n, a = C.c_void_p(), C.c_uint32(), C.c_void_p()
    one = (C.c_void_p * 1)(None)
    info = _lib.GroupInfoC()
    out, cnt, n_max = (C.c_float * 8)(), (C.c_int32 * 1)(), C.c_uint64()
    ix = (C.c_uint32 * 1)(0)
    calls = [
        lambda: L.bdr_candle_dqn_group_create(None, 1, C.byref(g)),
        lambda: L.bdr_candle_dqn_group_create(one, 1, None),
        lambda: L.bdr_candle_dqn_group_size(None, C.byref(n)),
        lambda: L.bdr_candle_dqn_group_member(None, 0, C.byref(a)),
        lambda: L.bdr_candle_dqn_group_info(None, C.byref(info)),
        lambda: L.bdr_candle_dqn_group_opt(None, one),
        lambda: L.bdr_candle_dqn_group_opt_with_scalars(None, one, out, 8, cnt),
        lambda: L.bdr_candle_dqn_group_sync(None),
        lambda: L.bdr_candle_dqn_group_sample(None, None, 1, one, cnt, one),
        lambda: L.bdr_candle_dqn_group_sample_members(None, ix, 1, None, 1, one, cnt, one),
        lambda: L.bdr_candle_dqn_group_last_q(None, 0, out, 8),
        lambda: L.bdr_candle_dqn_group_push(None, one, 1, one, one, None, one, one, one, one),
        lambda: L.bdr_candle_dqn_group_push_max_rows(None, one, None, C.byref(n_max)),
    ]
    for k, call in enumerate(calls):
        assert call() == INVALID, k
        assert b"null" in L.bdr_last_error(), (k, L.bdr_last_error())
    assert L.bdr_candle_dqn_group_destroy(None) == 0            # destroying nothing is no error, as for the other groups
    # the default tables of a NULL group: filled, naming no members; NULL tables are left alone
    ops, ev, post = _lib.GroupTrainerOps(), _lib.GroupEvalOps(), _lib.GroupTrainerPostC()
    L.bdr_candle_dqn_group_trainer_ops_default(C.byref(ops), None, None)
    L.bdr_candle_dqn_group_eval_ops_default(C.byref(ev), None)
    L.bdr_candle_dqn_group_trainer_post_default(C.byref(post), None)
    assert ops.n_members == 0 and ev.n_members == 0 and post.eval_ops.n_members == 0
    assert all(getattr(ops, f) for f in ("set_train", "sample", "push", "opt", "opt_with_record")) and ev.sample_members and post.save_member
    L.bdr_candle_dqn_group_trainer_ops_default(None, None, None)
    L.bdr_candle_dqn_group_eval_ops_default(None, None)
    L.bdr_candle_dqn_group_trainer_post_default(None, None)


def test_what_create_refuses_before_it_looks_for_a_device(L):
    g = C.c_void_p()
    one = (C.c_void_p * 1)(None)
    assert L.bdr_candle_dqn_group_create(one, 0, C.byref(g)) == INVALID and b"1 .. 65535 members" in L.bdr_last_error()
    assert L.bdr_candle_dqn_group_create(one, 65536, C.byref(g)) == INVALID and b"1 .. 65535 members" in L.bdr_last_error()
    assert L.bdr_candle_dqn_group_create(one, 1, C.byref(g)) == INVALID and b"member 0: null agent" in L.bdr_last_error()
    assert not g.value


def test_without_a_device_no_member_can_be_built(L):
    import border_amd as B
    from border_amd.iql import CandleMlpConfig
    cfg = B.CandleDqnConfig(obs_dim=4, n_actions=2, model_config=B.CandleDqnModelConfig(CandleMlpConfig((64, 64))), batch_size=8, device=0)
    if _lib.device_count() > 0:
        g = B.CandleDqnGroup.build([cfg])      # with one, a group of one exists and says what it is
        assert g.form == "candle_dqn_layers" and g.launches_per_round == 10 and len(g) == 1
        g.close()
        return
    with pytest.raises(B.BdrError) as e:
        B.CandleDqnGroup.build([cfg])
    assert e.value.code == 2   # BDR_ERR_NO_DEVICE (the refusals that need members: tests/test_gpu_candle_dqn_group.py)
