"""CPU tests of the range search's boundary: vrod_range_search and vrod_range_search_device are declared in
include/vrod.h with the documented argument types, exported by the built library, bound in Python and in the Rust text;
the three agree on VROD_ERR_CAPACITY = 8; and Python rejects a threshold array of the wrong length or a NaN threshold
before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vrod_range_search", "vrod_range_search_device"]


def header():
    return open(os.path.join(ROOT, "include", "vrod.h")).read()


def test_header_declares_the_entry_points_with_the_documented_arguments():
    src = re.sub(r"\s+", " ", header())
    assert ("int vrod_range_search(vrod_index *idx, const float *queries, uint32_t nq, const float *thresholds, "
            "uint64_t capacity, uint64_t *out_lims, uint64_t *out_ids, float *out_scores);") in src
    assert ("int vrod_range_search_device(vrod_index *idx, const float *d_queries, uint32_t nq, const float *d_thresholds, "
            "uint64_t capacity, uint64_t *d_out_lims, uint64_t *d_out_ids, float *d_out_scores, void *stream);") in src


def test_library_exports_and_python_binds_them():
    from vrod_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _lib.load()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    for name in NAMES:
        assert name in exported and name in _lib.SYMBOLS
        assert getattr(L, name).restype is C.c_int
    assert L.vrod_range_search.argtypes == [vp, vp, u32, vp, u64, vp, vp, vp]
    assert L.vrod_range_search_device.argtypes == [vp, vp, u32, vp, u64, vp, vp, vp, vp]
    # a null handle is refused before anything else is looked at
    lims = (u64 * 1)()
    assert L.vrod_range_search(None, None, 0, None, 0, lims, None, None) == 1
    assert L.vrod_range_search_device(None, None, 0, None, 0, lims, None, None, None) == 1


def test_err_capacity_is_8_everywhere():
    from vrod_amd import _lib
    assert re.search(r"VROD_ERR_CAPACITY\s*=\s*8\b", header())
    assert _lib.ERR_CAPACITY == 8
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"pub const VROD_ERR_CAPACITY: c_int = 8;", rust)
    for name in NAMES:
        assert re.search(r"pub fn %s\s*\(" % name, rust)


class _NoDevice:
    """An Index without a handle: the argument checks run before the library is called."""
    dim = 4


@pytest.mark.parametrize("threshold, what", [(np.zeros(3, np.float32), "3"), (np.float32("nan"), "NaN"),
                                             (np.array([0.1, np.nan], np.float32), "NaN")])
def test_python_validates_thresholds_without_a_device(threshold, what):
    from vrod_amd.index import Index
    ix = Index.__new__(Index)
    ix.dim = 4
    ix._h = None
    ix._L = None   # any call into the library would raise AttributeError, not ValueError
    with pytest.raises(ValueError, match=what):
        ix.range_search(np.zeros((2, 4), np.float32), threshold)
