"""CPU tests of the grouped-search entry points (vrod_search_grouped, vrod_search_grouped_device): exported, prototyped,
declared in the Rust crate, wrapped in Python, and their argument validation that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vrod_search_grouped", "vrod_search_grouped_device")


def test_symbols_are_declared_exported_and_prototyped():
    import vrod_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrod.h")).read(), flags=re.S)
    L = vrod_amd.load()
    out = subprocess.run(["nm", "-D", "--defined-only", vrod_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in vrod_amd.SYMBOLS
        assert re.search(rf" T {name}$", out, flags=re.M), name
        assert getattr(L, name).restype is C.c_int
    vp, u32 = C.c_void_p, C.c_uint32
    assert L.vrod_search_grouped.argtypes == [vp, vp, u32, u32, vp, vp, vp]
    assert L.vrod_search_grouped_device.argtypes == [vp, vp, u32, u32, vp, vp, vp, vp]


def test_rust_crate_declares_them():
    src = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    for name in NAMES:
        m = re.search(rf"pub fn {name}\s*\(([^;]*)\) -> c_int;", ext)
        assert m, name
        assert "out_labels: *mut u32" in m.group(1)
    assert "stream: *mut c_void" in re.search(r"pub fn vrod_search_grouped_device\s*\(([^;]*)\)", ext).group(1)


def test_argument_validation_without_device():
    import vrod_amd
    L = vrod_amd.load()
    q = (C.c_float * 4)()
    ids = (C.c_uint64 * 4)()
    sc = (C.c_float * 4)()
    lab = (C.c_uint32 * 4)()
    assert L.vrod_search_grouped(None, q, 1, 1, ids, sc, lab) == 1
    assert L.vrod_search_grouped(None, None, 1, 1, None, None, None) == 1
    assert L.vrod_search_grouped_device(None, q, 1, 1, ids, sc, lab, None) == 1
    assert L.vrod_search_grouped_device(None, None, 1, 1, None, None, None, None) == 1
    assert L.vrod_last_error()


def test_python_wrappers_exist_and_check_the_queries():
    import vrod_amd
    assert callable(vrod_amd.Index.search_grouped) and callable(vrod_amd.Index.search_grouped_device)
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    with pytest.raises(ValueError):
        ix.search_grouped(np.zeros((3, 5), np.float32), 2)
