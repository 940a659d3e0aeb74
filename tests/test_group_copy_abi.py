"""The hyperparameter and member-copy entry points of the C ABI without a GPU: the symbols are exported, the Python names map onto the
header's BDR_HYPER_* ids, and without a device the agents and groups the calls need cannot exist - their constructors fail with
BDR_ERR_NO_DEVICE - while a NULL handle is BDR_ERR_INVALID."""
import ctypes as C
import os
import re

import pytest

from border_amd import _lib, build

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "border_amd.h")
NEW = ("bdr_agent_hyper_get", "bdr_agent_hyper_set", "bdr_bc_group_copy_members", "bdr_iql_group_copy_members", "bdr_awac_group_copy_members",
       "bdr_candle_sac_group_copy_members")


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_the_new_symbols_are_exported_and_declared(L):
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"BDR_API int32_t %s\(" % name, text), name
        assert name in _lib.ABI_SYMBOLS, name


def test_python_names_are_the_headers_ids():
    text = open(HEADER).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"BDR_HYPER_(\w+) = (\d+)", text)}
    assert len(ids) == 27
    assert _lib.HYPER_IDS == ids   # "lr_actor" is BDR_HYPER_LR_ACTOR, "actor_beta1" BDR_HYPER_ACTOR_BETA1 ...
    assert _lib.BDR_COPY_HYPER == int(re.search(r"#define BDR_COPY_HYPER (\d+)", text).group(1))
    with pytest.raises(ValueError, match="unknown hyperparameter"):
        _lib.hyper_id("learning_rate")


def test_null_handles_are_invalid(L):
    v = C.c_double(0.0)
    assert L.bdr_agent_hyper_get(None, 0, C.byref(v)) == 1      # BDR_ERR_INVALID
    assert L.bdr_agent_hyper_set(None, 0, 1e-3) == 1
    ix = (C.c_uint32 * 1)(0)
    for k in ("bc", "iql", "awac", "candle_sac"):
        assert getattr(L, f"bdr_{k}_group_copy_members")(None, ix, ix, 1, 0) == 1
        assert b"null" in L.bdr_last_error()


def test_without_a_device_nothing_the_calls_need_can_be_built(L):
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    import border_amd as B
    for cls, cfg in ((B.Bc, B.BcConfig(obs_dim=4, act_dim=2, batch_size=8, action_type="Continuous", device=0)),
                     (B.Iql, B.IqlConfig(obs_dim=4, act_dim=2, batch_size=8, device=0)),
                     (B.Awac, B.AwacConfig(obs_dim=4, act_dim=2, batch_size=8, device=0)),
                     (B.CandleSac, B.CandleSacConfig(obs_dim=4, act_dim=2, batch_size=8, device=0))):
        with pytest.raises(B.BdrError) as e:
            cls.build(cfg)
        assert e.value.code == 2   # BDR_ERR_NO_DEVICE
    for grp, cfgs in ((B.BcGroup, [B.BcConfig(obs_dim=4, act_dim=2, batch_size=8, action_type="Continuous", device=0)] * 2),):
        with pytest.raises(B.BdrError) as e:
            grp.build(cfgs)
        assert e.value.code == 2
