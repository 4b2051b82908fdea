"""CPU tests of the row-value entry points (vrod_index_set_values, vrod_index_get_values, vrod_search_where,
vrod_search_where_device): the four names in every layer, the predicate struct's size, argument validation that needs no
device, and the Python wrappers' own checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vrod_index_set_values", "vrod_index_get_values", "vrod_search_where", "vrod_search_where_device"]
vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
ARGTYPES = {
    "vrod_index_set_values": [vp, u64, vp, u64],
    "vrod_index_get_values": [vp, u64, u64, vp],
    "vrod_search_where": [vp, vp, u32, u32, vp, vp, vp],
    "vrod_search_where_device": [vp, vp, u32, u32, vp, vp, vp, vp],
}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def test_names_in_every_layer():
    import vrod_amd
    L = vrod_amd.load()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in vrod.h"
        assert name in vrod_amd.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported"
        assert list(getattr(L, name).argtypes) == ARGTYPES[name], name
        assert getattr(L, name).restype in (C.c_int, C.c_int32), name
        assert re.search(r"\bpub fn %s\s*\(" % name, rust), f"{name} is not in the Rust binding"
    assert re.search(r"typedef struct\s*\{\s*uint64_t any, all, none;\s*int64_t lo, hi;\s*\}\s*vrod_where;", header)
    assert re.search(r"#\[repr\(C\)\][^{}]*pub struct vrod_where\s*\{\s*pub any: u64,\s*pub all: u64,\s*pub none: u64,\s*pub lo: i64,\s*pub hi: i64,\s*\}", rust)
    assert re.search(r"const int64_t \*values", header) and re.search(r"values: \*const i64", rust)   # signed in both
    for method in ("set_values", "get_values", "search_where", "search_where_device"):
        assert callable(getattr(vrod_amd.Index, method))


def test_predicate_struct_is_40_bytes(tmp_path):
    import vrod_amd
    assert vrod_amd.WHERE_DTYPE.itemsize == 40 and vrod_amd.WHERE_DTYPE.names == ("any", "all", "none", "lo", "hi")
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_where) == 40, "vrod_where");\n'
                   '_Static_assert(offsetof(vrod_where, lo) == 24 && offsetof(vrod_where, hi) == 32, "the interval follows the masks");\n'
                   'int main(void) { vrod_where w = {0, 0, 0, -1, 1}; return w.lo < 0 && w.lo < w.hi ? 0 : 1; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)                         # the ends are signed


def test_where_argument_validation_without_device():
    import vrod_amd
    L = vrod_amd.load()
    buf = (C.c_int64 * 4)()
    preds = (C.c_uint64 * 5)()
    q = (C.c_float * 4)()
    ids = (C.c_uint64 * 4)()
    sc = (C.c_float * 4)()
    assert L.vrod_index_set_values(None, 0, buf, 4) == 1
    assert L.vrod_index_set_values(None, 0, None, 0) == 1
    assert L.vrod_index_get_values(None, 0, 4, buf) == 1
    assert L.vrod_index_get_values(None, 0, 0, None) == 1
    for k in (1, 0, 3585):                                                       # a null handle is refused whatever k is
        assert L.vrod_search_where(None, q, 1, k, preds, ids, sc) == 1
        assert L.vrod_search_where_device(None, q, 1, k, preds, ids, sc, None) == 1
    assert L.vrod_search_where(None, None, 1, 1, None, None, None) == 1
    assert L.vrod_search_where_device(None, None, 1, 1, None, None, None, None) == 1
    assert L.vrod_last_error()


def test_wrappers_reject_bad_value_arrays():
    import vrod_amd
    f = vrod_amd.Index._i64
    with pytest.raises(TypeError):
        f(np.zeros(4, np.float32), "values")
    with pytest.raises(TypeError):
        f(np.zeros(4, bool), "values")
    with pytest.raises(ValueError):
        f(np.array([1 << 63], np.uint64), "values")
    a = f(np.array([[-1, 2], [I64_MIN, I64_MAX]], np.int64), "values")
    assert a.dtype == np.int64 and a.tolist() == [-1, 2, I64_MIN, I64_MAX] and a.flags.c_contiguous
    assert f([-5, 5], "values").tolist() == [-5, 5] and f(np.array([7], np.uint32), "values").dtype == np.int64
    assert f([], "values").size == 0 and f([], "values").dtype == np.int64


def test_predicate_forms():
    import vrod_amd
    W, DT = vrod_amd.Index._where, vrod_amd.WHERE_DTYPE
    s = np.array([(1 << 63, 0, 3, I64_MIN, -1), (0, 0, 0, -5, I64_MAX)], DT)
    assert W(s, 2) is s or np.array_equal(W(s, 2), s)
    p = W([[1 << 63, 0, 3, I64_MIN, -1], [0, 0, 0, -5, I64_MAX]], 2)             # Python ints keep both ranges
    assert p.dtype == DT and p.flags.c_contiguous and np.array_equal(p, s)
    p = W(np.array([[1, 2, 4, -5, 5]], np.int64), 1)                             # an int64 array: the ends are signed
    assert p.tolist() == [(1, 2, 4, -5, 5)]
    assert p.view(np.uint64).tolist() == [1, 2, 4, (1 << 64) - 5, 5]             # the bytes the library reads
    assert W(np.array([[1 << 63, 0, 0, 0, 9]], np.uint64), 1).tolist() == [(1 << 63, 0, 0, 0, 9)]
    assert W([], 0).size == 0 and W(np.zeros((0, 5), np.int64), 0).dtype == DT
    for bad, err in (([[-1, 0, 0, 0, 0]], ValueError), ([[0, 0, 0, 1 << 63, 0]], ValueError), ([[0, 0, 0, 0, I64_MIN - 1]], ValueError),
                     (np.array([[0, -1, 0, 0, 0]], np.int64), ValueError), (np.array([[0, 0, 0, 0, 1 << 63]], np.uint64), ValueError),
                     (np.zeros((1, 5), np.float64), TypeError), ([[0.5, 0, 0, 0, 0]], TypeError), (np.zeros((1, 3), np.uint64), ValueError),
                     (np.zeros(5, np.int64), ValueError), (np.zeros(1, np.dtype([("any", np.uint64), ("lo", np.int64)])), TypeError)):
        with pytest.raises(err):
            W(bad, 1)
    with pytest.raises(ValueError):
        W(s, 3)                                                                  # one predicate per query


def test_search_where_checks_predicates_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    q = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError):
        ix.search_where(q, 2, np.zeros((2, 5), np.int64))
    with pytest.raises(ValueError):
        ix.search_where(q, 2, np.zeros((3, 3), np.uint64))
    with pytest.raises(TypeError):
        ix.search_where(q, 2, np.zeros((3, 5), np.float64))
