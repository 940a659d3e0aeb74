"""The agent-group entry points exist: declared in include/border_amd.h, exported by the built library, checked arguments, and
the Python mirror imports.  No compute calls: runs without a GPU."""
import ctypes as C
import os
import re

import pytest

from border_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUP_SYMBOLS = ["bdr_agent_group_create", "bdr_agent_group_destroy", "bdr_agent_group_size", "bdr_agent_group_member",
                 "bdr_agent_group_opt", "bdr_agent_group_opt_with_scalars", "bdr_agent_group_qvalues", "bdr_agent_group_sample",
                 "bdr_agent_group_sync"]
BDR_ERR_INVALID = 1


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_the_nine_symbols_are_declared_and_exported(L):
    hdr = open(os.path.join(ROOT, "include", "border_amd.h")).read()
    declared = set(re.findall(r"BDR_API[^;(]*?\b(bdr_[a-z0-9_]+)\s*\(", hdr))
    assert "typedef struct bdr_agent_group bdr_agent_group;" in hdr
    for s in GROUP_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in _lib.ABI_SYMBOLS, s


def test_null_arguments_are_invalid(L):
    out = C.c_void_p()
    n = C.c_uint32()
    one = (C.c_void_p * 1)(None)
    assert L.bdr_agent_group_create(None, 1, C.byref(out)) == BDR_ERR_INVALID
    assert L.bdr_agent_group_create(one, 1, None) == BDR_ERR_INVALID
    assert L.bdr_agent_group_create(one, 0, C.byref(out)) == BDR_ERR_INVALID       # an empty group
    assert L.bdr_agent_group_create(one, 1, C.byref(out)) == BDR_ERR_INVALID       # a null member
    assert b"member 0" in L.bdr_last_error()
    assert out.value is None
    assert L.bdr_agent_group_size(None, C.byref(n)) == BDR_ERR_INVALID
    assert L.bdr_agent_group_member(None, 0, C.byref(out)) == BDR_ERR_INVALID
    assert L.bdr_agent_group_opt(None, one) == BDR_ERR_INVALID
    assert L.bdr_agent_group_opt_with_scalars(None, one, None, 1, None) == BDR_ERR_INVALID
    assert L.bdr_agent_group_qvalues(None, one, one) == BDR_ERR_INVALID
    assert L.bdr_agent_group_sample(None, one, None, None) == BDR_ERR_INVALID
    assert L.bdr_agent_group_sync(None) == BDR_ERR_INVALID
    assert L.bdr_agent_group_destroy(None) == 0                                    # like bdr_agent_destroy(NULL)


def test_the_python_mirror_imports():
    import border_amd
    from border_amd.group import DqnGroup
    assert border_amd.DqnGroup is DqnGroup
    for m in ("build", "members", "opt", "opt_with_record", "sample", "qvalues", "close"):
        assert hasattr(DqnGroup, m), m
    assert DqnGroup.STAGING_DEPTH >= 1
