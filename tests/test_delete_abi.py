"""CPU tests of row deletion's boundary: vrod_index_delete and vrod_index_live_count are declared in include/vrod.h,
exported by the library and bound in Python and Rust, and refuse a null handle without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrod_index_delete", "vrod_index_live_count")


def _header():
    src = open(os.path.join(ROOT, "include", "vrod.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    assert re.search(r"int vrod_index_delete\(vrod_index \*idx, const uint64_t \*ids, uint64_t n\);", src)
    assert re.search(r"int vrod_index_live_count\(const vrod_index \*idx, uint64_t \*out\);", src)


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
    assert len(L.vrod_index_delete.argtypes) == 3 and len(L.vrod_index_live_count.argtypes) == 2
    assert callable(vrod_amd.Index.delete) and callable(vrod_amd.Index.live_count)


def test_rust_binding_declares_and_wraps():
    src = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    assert re.search(r"pub fn vrod_index_delete\(idx: \*mut vrod_index, ids: \*const u64, n: u64\) -> c_int;", ext)
    assert re.search(r"pub fn vrod_index_live_count\(idx: \*const vrod_index, out: \*mut u64\) -> c_int;", ext)
    assert re.search(r"pub fn delete\(&mut self, ids: &\[u64\]\) -> Result<\(\), ScanError>", src)
    assert re.search(r"pub fn live_len\(&self\) -> u64", src)


def test_null_handle_is_invalid_arg_without_device():
    import vrod_amd
    L = vrod_amd.load()
    ids = (C.c_uint64 * 2)(0, 1)
    out = C.c_uint64(7)
    assert L.vrod_index_delete(None, ids, 2) == 1
    assert L.vrod_index_delete(None, None, 0) == 1
    assert L.vrod_index_live_count(None, C.byref(out)) == 1
    assert out.value == 7
    assert L.vrod_last_error()


def test_python_delete_rejects_non_integer_ids():
    import vrod_amd
    idx = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the argument conversion runs
    with pytest.raises(TypeError):
        idx.delete(np.array([0.5, 1.0]))
