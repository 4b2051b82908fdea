"""CPU tests of the allow-list filter's boundary: vrod_index_set_filter and vrod_index_filter_count are declared in
include/vrod.h with VROD_PATH_GATHER, exported by the library and bound in Python and Rust, and refuse a null handle
without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrod_index_set_filter", "vrod_index_filter_count")


def _header():
    src = open(os.path.join(ROOT, "include", "vrod.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_points_and_the_path():
    src = _header()
    assert re.search(r"int vrod_index_set_filter\(vrod_index \*idx, const uint32_t \*allow_words, uint64_t n_rows\);", src)
    assert re.search(r"int vrod_index_filter_count\(const vrod_index \*idx, uint64_t \*out\);", src)
    assert re.search(r"VROD_PATH_GATHER = 4", src)


def test_library_exports_and_python_binds():
    import vrod_amd
    from vrod_amd import _lib
    for name in NEW:
        assert name in _lib.SYMBOLS
    L = vrod_amd.load()
    out = subprocess.run(["nm", "-D", "--defined-only", vrod_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vrod_[a-z_0-9]+)", out))
    for name in NEW:
        assert name in exported
        assert getattr(L, name).restype is C.c_int
    assert len(L.vrod_index_set_filter.argtypes) == 3 and len(L.vrod_index_filter_count.argtypes) == 2
    assert callable(vrod_amd.Index.set_filter) and callable(vrod_amd.Index.filter_count)
    assert vrod_amd.PATH_GATHER == 4


def test_rust_binding_declares_and_wraps():
    src = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    assert re.search(r"pub fn vrod_index_set_filter\(idx: \*mut vrod_index, allow_words: \*const u32, n_rows: u64\) -> c_int;", ext)
    assert re.search(r"pub fn vrod_index_filter_count\(idx: \*const vrod_index, out: \*mut u64\) -> c_int;", ext)
    assert re.search(r"pub fn set_filter\(&mut self, allowed: Option<&\[bool\]>\) -> Result<\(\), ScanError>", src)
    assert re.search(r"pub fn filter_len\(&self\) -> u64", src)
    assert re.search(r"pub const VROD_PATH_GATHER: c_int = 4;", src)


def test_null_handle_is_invalid_arg_without_device():
    import vrod_amd
    L = vrod_amd.load()
    words = (C.c_uint32 * 2)(0xFFFFFFFF, 1)
    out = C.c_uint64(7)
    assert L.vrod_index_set_filter(None, words, 33) == 1
    assert L.vrod_index_set_filter(None, None, 0) == 1
    assert L.vrod_index_filter_count(None, C.byref(out)) == 1
    assert out.value == 7
    assert L.vrod_index_set_path(None, 4) == 1
    assert L.vrod_last_error()


def test_python_set_filter_rejects_non_bool():
    import vrod_amd
    idx = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the argument conversion runs
    with pytest.raises(TypeError):
        idx.set_filter(np.array([0, 1, 1]))
