"""CPU tests of the boundary of the two corpus mutations: vrod_index_update and vrod_index_compact are declared in
include/vrod.h, exported by the library and bound in Python and Rust, and refuse a null handle without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vrod_index_update", "vrod_index_compact")


def _header():
    src = open(os.path.join(ROOT, "include", "vrod.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    assert re.search(r"int vrod_index_update\(vrod_index \*idx, const uint64_t \*ids, const float \*rows, uint64_t n\);", src)
    assert re.search(r"int vrod_index_compact\(vrod_index \*idx, uint64_t \*out_new_ids, uint64_t map_len\);", src)


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
    assert len(L.vrod_index_update.argtypes) == 4 and len(L.vrod_index_compact.argtypes) == 3
    assert callable(vrod_amd.Index.update) and callable(vrod_amd.Index.compact)


def test_rust_binding_declares_and_wraps():
    src = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    assert re.search(r"pub fn vrod_index_update\(idx: \*mut vrod_index, ids: \*const u64, rows: \*const f32, n: u64\) -> c_int;", ext)
    assert re.search(r"pub fn vrod_index_compact\(idx: \*mut vrod_index, out_new_ids: \*mut u64, map_len: u64\) -> c_int;", ext)
    assert re.search(r"pub fn update\(&mut self, ids: &\[u64\], embeddings: &\[Vec<f32>\]\) -> Result<\(\), ScanError>", src)
    assert re.search(r"pub fn compact\(&mut self\) -> Result<Vec<u64>, ScanError>", src)


def test_null_handle_is_invalid_arg_without_device():
    import vrod_amd
    L = vrod_amd.load()
    ids = (C.c_uint64 * 2)(0, 1)
    rows = (C.c_float * 8)()
    new_ids = (C.c_uint64 * 2)(7, 7)
    assert L.vrod_index_update(None, ids, rows, 2) == 1
    assert L.vrod_index_update(None, None, None, 0) == 1
    assert L.vrod_index_compact(None, new_ids, 2) == 1
    assert L.vrod_index_compact(None, None, 0) == 1
    assert list(new_ids) == [7, 7]
    assert L.vrod_last_error()


def test_python_update_checks_its_arguments():
    import vrod_amd
    idx = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the argument conversion runs
    idx.dim = 4
    with pytest.raises(TypeError):
        idx.update(np.array([0.5]), np.zeros((1, 4), np.float32))
    with pytest.raises(ValueError):
        idx.update([1, 2], np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError):
        idx.update([1, 2], np.zeros((2, 5), np.float32))


def test_mutation_kernels_leave_the_scan_kernels_alone():
    """Neither feature touches a scan kernel: the new device code lives in a file of its own."""
    csrc = os.path.join(ROOT, "vrod_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_mutate.hip" in mk and "compact_plan.h" in mk
    src = open(os.path.join(csrc, "kernels_mutate.hip")).read()
    for name in ("scatter_rows_kernel", "compact_rows_kernel", "launch_scatter_rows", "launch_compact_rows"):
        assert name in src
    assert "mfma" not in src.lower()
