"""CPU tests of the multi-vector search entry points (vrod_search_multivec, vrod_search_multivec_device,
vrod_index_last_multivec): exported, prototyped, declared in the Rust crate, wrapped in Python, and the argument
validation that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vrod_search_multivec", "vrod_search_multivec_device", "vrod_index_last_multivec")


def test_symbols_are_declared_exported_and_prototyped():
    import vrod_amd
    raw = open(os.path.join(ROOT, "include", "vrod.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = vrod_amd.load()
    out = subprocess.run(["nm", "-D", "--defined-only", vrod_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in vrod_amd.SYMBOLS
        assert re.search(rf" T {name}$", out, flags=re.M), name
        assert getattr(L, name).restype is C.c_int
    assert re.search(r"#define VROD_MAX_QUERY_VECTORS 256u", hdr)
    vp, u32 = C.c_void_p, C.c_uint32
    assert L.vrod_search_multivec.argtypes == [vp, vp, vp, u32, u32, vp, vp, vp]
    assert L.vrod_search_multivec_device.argtypes == [vp, vp, vp, u32, u32, vp, vp, vp, vp]
    # the stats struct: five words, padding, two 64-bit counters -- as the header declares it
    from vrod_amd._lib import MultivecStats
    m = re.search(r"typedef struct \{([^}]*)\} vrod_multivec_stats;", hdr)
    fields = [f.strip() for part in m.group(1).split(";") if part.strip() for f in part.strip().split(" ", 1)[1].split(",")]
    assert fields == [n for n, _ in MultivecStats._fields_]
    assert C.sizeof(MultivecStats) == 40 and MultivecStats.candidate_labels.offset == 24


def test_rust_crate_declares_them():
    src = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    for name in NAMES:
        assert re.search(rf"pub fn {name}\s*\(([^;]*)\) -> c_int;", ext), name
    args = re.search(r"pub fn vrod_search_multivec_device\s*\(([^;]*)\)", ext).group(1)
    assert "d_query_lims: *const u32" in args and "d_out_found: *mut u32" in args and "stream: *mut c_void" in args
    assert "query_lims: *const u32" in re.search(r"pub fn vrod_search_multivec\s*\(([^;]*)\)", ext).group(1)
    st = re.search(r"pub struct vrod_multivec_stats \{(.*?)\n\}", src, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", st) == [("nq", "u32"), ("vectors", "u32"), ("k1", "u32"), ("certified_queries", "u32"),
                                                     ("dense_queries", "u32"), ("candidate_labels", "u64"), ("candidate_rows", "u64")]
    assert "pub const VROD_MAX_QUERY_VECTORS: u32 = 256;" in src


def test_argument_validation_without_device():
    import vrod_amd
    from vrod_amd._lib import MultivecStats
    L = vrod_amd.load()
    v = (C.c_float * 4)()
    lims = (C.c_uint32 * 2)(0, 1)
    lab = (C.c_uint32 * 4)()
    sc = (C.c_float * 4)()
    fnd = (C.c_uint32 * 1)()
    assert L.vrod_search_multivec(None, v, lims, 1, 1, lab, sc, fnd) == 1
    assert L.vrod_search_multivec(None, None, None, 1, 1, None, None, None) == 1
    assert L.vrod_search_multivec_device(None, v, lims, 1, 1, lab, sc, fnd, None) == 1
    assert L.vrod_search_multivec_device(None, None, None, 0, 1, None, None, None, None) == 1
    assert L.vrod_index_last_multivec(None, C.byref(MultivecStats())) == 1
    assert L.vrod_last_error()


def test_python_wrappers_exist_and_check_their_shapes():
    import vrod_amd
    assert callable(vrod_amd.Index.search_multivec) and callable(vrod_amd.Index.search_multivec_device)
    assert callable(vrod_amd.Index.last_multivec)
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    with pytest.raises(ValueError):
        ix.search_multivec([np.zeros((3, 5), np.float32)], 2)                       # a query of the wrong width
    with pytest.raises(ValueError):
        ix.search_multivec(np.zeros((3, 5), np.float32), 2, lims=[0, 3])            # vectors of the wrong width
    with pytest.raises(ValueError):
        ix.search_multivec(np.zeros((3, 4), np.float32), 2, lims=[0, 2])            # lims do not cover the vectors
    with pytest.raises(ValueError):
        ix.search_multivec(np.zeros((3, 4), np.float32), 2, lims=[[0, 3]])          # lims not a vector
    with pytest.raises(ValueError):
        ix.search_multivec(np.zeros((3, 4), np.float32), 2, lims=[0.0, 3.0])        # lims not integers
    v, la = ix._multivec_args([np.zeros((2, 4)), np.zeros(4), np.zeros((3, 4))], None)
    assert v.shape == (6, 4) and v.dtype == np.float32 and la.tolist() == [0, 2, 3, 6] and la.dtype == np.uint32
