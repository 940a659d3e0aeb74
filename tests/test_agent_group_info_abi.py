"""bdr_agent_group_info without a GPU: declared in include/border_amd.h, exported by the library, listed in _lib.ABI_SYMBOLS and in the
Rust shim; NULL arguments are BDR_ERR_INVALID; the struct the header declares has the layout of the ctypes mirror."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from border_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "border_amd.h")


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def test_declared_exported_and_listed(L):
    hdr = open(HEADER).read()
    assert re.search(r"BDR_API\s+int32_t\s+bdr_agent_group_info\s*\(\s*const\s+bdr_agent_group\s*\*\s*g\s*,\s*bdr_group_info\s*\*\s*out\s*\)\s*;", hdr)
    assert re.search(r"#define\s+BDR_GROUP_FORM_ONE_WORKGROUP\s+0\b", hdr) and re.search(r"#define\s+BDR_GROUP_FORM_LAYERS\s+1\b", hdr)
    assert hasattr(L, "bdr_agent_group_info")
    assert "bdr_agent_group_info" in _lib.ABI_SYMBOLS
    assert (_lib.GROUP_FORM_ONE_WORKGROUP, _lib.GROUP_FORM_LAYERS) == (0, 1)
    ffi = open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "ffi.rs")).read()
    assert "pub fn bdr_agent_group_info(g: *const bdr_agent_group, out: *mut bdr_group_info) -> i32;" in ffi
    assert "pub struct bdr_group_info" in ffi and "pub const BDR_GROUP_FORM_LAYERS: i32 = 1;" in ffi
    assert "ffi::bdr_agent_group_info" in open(os.path.join(ROOT, "rust", "border-amd-agent", "src", "group.rs")).read()
    assert "bdr_agent_group_info" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_are_invalid(L):
    info = _lib.GroupInfoC()
    assert L.bdr_agent_group_info(None, C.byref(info)) == 1   # BDR_ERR_INVALID
    assert b"null" in L.bdr_last_error()
    not_a_group = C.c_void_p(16)                             # (never dereferenced: the NULL output is refused first)
    assert L.bdr_agent_group_info(not_a_group, None) == 1
    assert L.bdr_agent_group_info(None, None) == 1


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = [f for f, _ in _lib.GroupInfoC._fields_]
    assert fields == ["form", "n_members", "launches_per_round", "reserved", "kernel_launches"]
    prog = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {", '  printf("%zu", sizeof(bdr_group_info));']
    prog += [f'  printf(" %zu", offsetof(bdr_group_info, {f}));' for f in fields]
    prog += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text("\n".join(prog))
    subprocess.check_call([cc, "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)])
    size, *offs = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(_lib.GroupInfoC) == 24
    assert offs == [getattr(_lib.GroupInfoC, f).offset for f in fields] == [0, 4, 8, 12, 16]
    assert (_lib.GroupInfoC.form.size, _lib.GroupInfoC.kernel_launches.size) == (4, 8)
