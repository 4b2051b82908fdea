"""CPU tests of the row-predicate entry points (vrod_index_count_where, _select_where, _select_where_device, _delete_where,
_set_filter_where, _set_tags_where): the six names in every layer, the predicate struct's size and offsets, argument
validation that needs no device, and the Python wrappers' own checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u32, u64, pu64 = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)
ARGTYPES = {
    "vrod_index_count_where": [vp, vp, u32, u32, vp],
    "vrod_index_select_where": [vp, vp, u32, u64, pu64, vp],
    "vrod_index_select_where_device": [vp, vp, u32, u64, pu64, vp, vp],
    "vrod_index_delete_where": [vp, vp, u32, pu64],
    "vrod_index_set_filter_where": [vp, vp, u32],
    "vrod_index_set_tags_where": [vp, vp, u32, u64, u64, pu64],
}
NAMES = list(ARGTYPES)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FIELDS = ("any", "all", "none", "lo", "hi", "label", "has_label")


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
    assert re.search(r"typedef struct\s*\{\s*uint64_t any, all, none;[^}]*int64_t\s+lo, hi;[^}]*uint32_t\s+label;[^}]*uint32_t\s+has_label;[^}]*\}\s*vrod_row_pred;", header)
    assert re.search(r"#\[repr\(C\)\][^{}]*pub struct vrod_row_pred\s*\{\s*pub any: u64,\s*pub all: u64,\s*pub none: u64,\s*pub lo: i64,\s*pub hi: i64,"
                     r"\s*pub label: u32,\s*pub has_label: u32,\s*\}", rust)
    assert re.search(r"#define VROD_ROWPRED_ALLOWED 1u", header) and re.search(r"pub const VROD_ROWPRED_ALLOWED: u32 = 1;", rust)
    assert vrod_amd.ROWPRED_ALLOWED == 1
    for method in ("count_where", "select_where", "select_where_device", "delete_where", "set_filter_where", "set_tags_where"):
        assert callable(getattr(vrod_amd.Index, method))
    typedef = header[header.index("} vrod_where;"):]
    assert "} vrod_where; /* 40 bytes, no padding */" in header and "vrod_row_pred" in typedef   # vrod_where keeps its layout


def test_predicate_struct_is_48_bytes(tmp_path):
    import vrod_amd
    DT = vrod_amd.ROWPRED_DTYPE
    assert DT.itemsize == 48 and DT.names == FIELDS
    assert [DT.fields[n][1] for n in FIELDS] == [0, 8, 16, 24, 32, 40, 44]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_row_pred) == 48, "vrod_row_pred");\n'
                   '_Static_assert(offsetof(vrod_row_pred, any) == 0 && offsetof(vrod_row_pred, all) == 8 && offsetof(vrod_row_pred, none) == 16, "the masks");\n'
                   '_Static_assert(offsetof(vrod_row_pred, lo) == 24 && offsetof(vrod_row_pred, hi) == 32, "the interval follows the masks");\n'
                   '_Static_assert(offsetof(vrod_row_pred, label) == 40 && offsetof(vrod_row_pred, has_label) == 44, "then the label");\n'
                   '_Static_assert(sizeof(vrod_where) == 40 && VROD_ROWPRED_ALLOWED == 1, "vrod_where keeps its layout");\n'
                   'int main(void) { vrod_row_pred p = {0, 0, 0, -1, 1, 0xFFFFFFFFu, 1}; return p.lo < 0 && p.lo < p.hi && p.label > 0 ? 0 : 1; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)                         # the ends are signed, the label is not


def test_argument_validation_without_device():
    """A null handle is refused by every entry point whatever else it is given -- null pointers, unknown flag bits,
    has_label == 2, set_bits & clear_bits != 0 -- and the outputs are not written."""
    import vrod_amd
    L = vrod_amd.load()
    good = np.zeros(1, vrod_amd.ROWPRED_DTYPE)
    good["lo"], good["hi"] = I64_MIN, I64_MAX
    bad_label = good.copy()
    bad_label["has_label"] = 2
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    n = C.c_uint64(7)
    for p in (good, bad_label, None):
        pp = p.ctypes.data_as(vp) if p is not None else None
        for flags in (0, 1, 2, 0xFFFFFFFF):
            assert L.vrod_index_count_where(None, pp, 1, flags, out) == 1
            assert L.vrod_index_count_where(None, pp, 0, flags, None) == 1
            assert L.vrod_index_select_where(None, pp, flags, 4, C.byref(n), out) == 1
            assert L.vrod_index_select_where(None, pp, flags, 0, None, None) == 1
            assert L.vrod_index_select_where_device(None, pp, flags, 4, C.byref(n), out, None) == 1
            assert L.vrod_index_delete_where(None, pp, flags, C.byref(n)) == 1
            assert L.vrod_index_delete_where(None, pp, flags, None) == 1
            assert L.vrod_index_set_filter_where(None, pp, flags) == 1
            for set_bits, clear_bits in ((1, 2), (3, 1), (0, 0)):
                assert L.vrod_index_set_tags_where(None, pp, flags, set_bits, clear_bits, C.byref(n)) == 1
    assert list(out) == [7, 7, 7, 7] and n.value == 7
    assert L.vrod_last_error()


def test_predicate_forms():
    import vrod_amd
    P, DT = vrod_amd.Index._row_preds, vrod_amd.ROWPRED_DTYPE
    s = np.array([(1 << 63, 0, 3, I64_MIN, -1, 0xFFFFFFFF, 1), (0, 0, 0, -5, I64_MAX, 0, 0)], DT)
    assert P(s, 2) is s or np.array_equal(P(s, 2), s)
    p = P([[1 << 63, 0, 3, I64_MIN, -1, 0xFFFFFFFF, 1], [0, 0, 0, -5, I64_MAX, 0, 0]], 2)   # Python ints keep every range
    assert p.dtype == DT and p.flags.c_contiguous and np.array_equal(p, s)
    assert np.array_equal(P(s), s) and P(s[0], 1).tolist() == [s[0].tolist()]    # any count; one struct
    p = P((1, 2, 4, -5, 5, 9, 1), 1)                                             # one predicate as its 7 values
    assert p.tolist() == [(1, 2, 4, -5, 5, 9, 1)]
    p = P(np.array([[1, 2, 4, -5, 5, 9, 1]], np.int64), 1)                        # an int64 array: the ends are signed
    assert p.tolist() == [(1, 2, 4, -5, 5, 9, 1)]
    assert p.view(np.uint8).size == 48 and p.view(np.uint64)[:5].tolist() == [1, 2, 4, (1 << 64) - 5, 5]   # the bytes the library reads
    assert p.view(np.uint32)[10:].tolist() == [9, 1]
    assert P([], 0).size == 0 and P(np.zeros((0, 7), np.int64), 0).dtype == DT
    for bad, err in (([[-1, 0, 0, 0, 0, 0, 0]], ValueError), ([[0, 0, 0, 1 << 63, 0, 0, 0]], ValueError), ([[0, 0, 0, 0, I64_MIN - 1, 0, 0]], ValueError),
                     ([[0, 0, 0, 0, 0, 1 << 32, 1]], ValueError), ([[0, 0, 0, 0, 0, -1, 1]], ValueError), ([[0, 0, 0, 0, 0, 0, 2]], ValueError),
                     (np.array([[0, -1, 0, 0, 0, 0, 0]], np.int64), ValueError), (np.array([[0, 0, 0, 0, 1 << 63, 0, 0]], np.uint64), ValueError),
                     (np.zeros((1, 7), np.float64), TypeError), ([[0.5, 0, 0, 0, 0, 0, 0]], TypeError), (np.zeros((1, 5), np.uint64), ValueError),
                     (np.zeros(6, np.int64), ValueError), (np.zeros(1, vrod_amd.WHERE_DTYPE), TypeError)):
        with pytest.raises(err):
            P(bad, 1)
    with pytest.raises(ValueError):
        P(s, 1)                                                                  # one predicate where one is wanted
    two = s.copy()
    two["has_label"][1] = 2
    with pytest.raises(ValueError):
        P(two)
    one = vrod_amd.Index.row_pred()
    assert one.tolist() == [(0, 0, 0, I64_MIN, I64_MAX, 0, 0)]                   # the defaults match every row
    assert vrod_amd.Index.row_pred(any=1 << 63, hi=-1, label=0).tolist() == [(1 << 63, 0, 0, I64_MIN, -1, 0, 1)]
    with pytest.raises(ValueError):
        vrod_amd.Index.row_pred(label=1 << 32)


def test_wrappers_check_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, None, 0
    ok = vrod_amd.Index.row_pred()
    two = np.concatenate([ok, ok])
    for call in (lambda p: ix.count_where(p), lambda p: ix.select_where(p), lambda p: ix.select_where_device(p, 4), lambda p: ix.delete_where(p),
                 lambda p: ix.set_filter_where(p), lambda p: ix.set_tags_where(p, 1, 2)):
        with pytest.raises(ValueError):
            call([[0, 0, 0, 0, 0, 0, 2]])                                        # has_label
        with pytest.raises(TypeError):
            call(np.zeros((1, 7), np.float64))
    for call in (lambda p: ix.select_where(p), lambda p: ix.delete_where(p), lambda p: ix.set_filter_where(p), lambda p: ix.set_tags_where(p, 1, 2)):
        with pytest.raises(ValueError):
            call(two)                                                            # one predicate per call
    with pytest.raises(TypeError):
        ix.count_where(ok, allowed_only=1)
    with pytest.raises(TypeError):
        ix.set_filter_where(ok, narrow="yes")
    with pytest.raises(ValueError):
        ix.set_tags_where(ok, 3, 1)                                              # set_bits & clear_bits
    with pytest.raises(ValueError):
        ix.set_tags_where(ok, -1, 0)
    with pytest.raises(ValueError):
        ix.set_tags_where(ok, 0, 1 << 64)
    with pytest.raises(TypeError):
        ix.set_tags_where(ok, 1.0, 0)
    with pytest.raises(ValueError):
        ix.select_where(ok, capacity=-1)
