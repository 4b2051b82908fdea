"""CPU tests of the ordered-selection entry points (vrod_index_select_ordered, _select_ordered_device): the two names in
every layer, the cursor struct's size and offsets, the two constants, argument validation that needs no device, and the
Python wrappers' own checks."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u32, u64, pu64 = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)
ARGTYPES = {
    "vrod_index_select_ordered": [vp, vp, u32, vp, u32, pu64, pu64, vp, vp],
    "vrod_index_select_ordered_device": [vp, vp, u32, vp, u32, pu64, pu64, vp, vp, vp],
}
NAMES = list(ARGTYPES)
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
    assert re.search(r"typedef struct\s*\{\s*int64_t value;\s*uint64_t id;\s*\}\s*vrod_order_cursor;", header)
    assert re.search(r"#\[repr\(C\)\][^{}]*pub struct vrod_order_cursor\s*\{\s*pub value: i64,\s*pub id: u64,\s*\}", rust)
    for method in ("select_ordered", "select_ordered_device", "scroll"):
        assert callable(getattr(vrod_amd.Index, method))


def test_the_two_constants_in_every_layer():
    import vrod_amd
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"#define VROD_ORDER_DESC\s+2u", header) and re.search(r"pub const VROD_ORDER_DESC: u32 = 2;", rust)
    assert re.search(r"#define VROD_MAX_ORDERED\s+65536u", header) and re.search(r"pub const VROD_MAX_ORDERED: u32 = 65536;", rust)
    assert vrod_amd.ORDER_DESC == 2 and vrod_amd.MAX_ORDERED == 65536
    assert vrod_amd.ORDER_DESC & vrod_amd.ROWPRED_ALLOWED == 0                   # they share the flags word


def test_cursor_struct_is_16_bytes(tmp_path):
    import vrod_amd
    DT = vrod_amd.ORDER_CURSOR_DTYPE
    assert DT.itemsize == 16 and DT.names == ("value", "id")
    assert [DT.fields[n][1] for n in DT.names] == [0, 8] and DT["value"] == np.int64 and DT["id"] == np.uint64
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_order_cursor) == 16, "vrod_order_cursor");\n'
                   '_Static_assert(offsetof(vrod_order_cursor, value) == 0 && offsetof(vrod_order_cursor, id) == 8, "value, then id");\n'
                   '_Static_assert(VROD_ORDER_DESC == 2 && VROD_MAX_ORDERED == 65536 && (VROD_ORDER_DESC & VROD_ROWPRED_ALLOWED) == 0, "the constants");\n'
                   'int main(void) { vrod_order_cursor c = {-1, 0xFFFFFFFFFFFFFFFFull}; return c.value < 0 && c.id > 0 ? 0 : 1; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)                         # the value is signed, the id is not


def test_argument_validation_without_device():
    """A null handle is refused by both forms for every combination of flags and pointers, and nothing is written."""
    import vrod_amd
    L = vrod_amd.load()
    good = np.zeros(1, vrod_amd.ROWPRED_DTYPE)
    good["lo"], good["hi"] = I64_MIN, I64_MAX
    bad_label = good.copy()
    bad_label["has_label"] = 2
    cur = np.zeros(1, vrod_amd.ORDER_CURSOR_DTYPE)
    ids, vals = (C.c_uint64 * 4)(7, 7, 7, 7), (C.c_int64 * 4)(7, 7, 7, 7)
    n, total = C.c_uint64(7), C.c_uint64(7)
    preds = [p.ctypes.data_as(vp) for p in (good, bad_label)] + [None]
    combos = itertools.product(preds, (0, 1, 2, 3, 4, 0xFFFFFFFF), (None, cur.ctypes.data_as(vp)), (0, 4, 65536, 65537), (None, C.byref(n)),
                               (None, C.byref(total)), (None, ids), (None, vals))
    seen = 0
    for pp, flags, after, limit, pn, pt, pi, pv in combos:
        assert L.vrod_index_select_ordered(None, pp, flags, after, limit, pn, pt, pi, pv) == 1
        assert L.vrod_index_select_ordered_device(None, pp, flags, after, limit, pn, pt, pi, pv, None) == 1
        seen += 1
    assert seen == 3 * 6 * 2 * 4 * 16
    assert list(ids) == [7] * 4 and list(vals) == [7] * 4 and n.value == 7 and total.value == 7
    assert L.vrod_last_error()


def test_wrappers_check_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, None, 0
    ok = vrod_amd.Index.row_pred()
    two = np.concatenate([ok, ok])
    calls = (lambda p, **kw: ix.select_ordered(p, kw.pop("limit", 5), **kw), lambda p, **kw: ix.select_ordered_device(p, kw.pop("limit", 5), **kw),
             lambda p, **kw: next(ix.scroll(p, kw.pop("limit", 5), **{k: v for k, v in kw.items() if k != "after"})))
    for call in calls:
        with pytest.raises(ValueError):
            call([[0, 0, 0, 0, 0, 0, 2]])                                        # has_label
        with pytest.raises(TypeError):
            call(np.zeros((1, 7), np.float64))
        with pytest.raises(ValueError):
            call(two)                                                            # one predicate per call
        for limit, err in ((-1, ValueError), (vrod_amd.MAX_ORDERED + 1, ValueError), (1 << 40, ValueError), (2.0, TypeError), ("5", TypeError), (True, TypeError),
                           (None, TypeError)):
            with pytest.raises(err):
                call(ok, limit=limit)
        with pytest.raises(TypeError):
            call(ok, desc=1)
        with pytest.raises(TypeError):
            call(ok, allowed_only="yes")
    with pytest.raises(ValueError):
        next(ix.scroll(ok, 0))                                                   # a page holds at least one row
    for call in calls[:2]:
        for after, err in (((1 << 63, 0), ValueError), ((I64_MIN - 1, 0), ValueError), ((0, -1), ValueError), ((0, 1 << 64), ValueError), ((0,), TypeError),
                           ((0, 1, 2), TypeError), (5, TypeError), ((0.5, 1), TypeError), ((0, 1.0), TypeError), ((True, 1), TypeError), ("ab", TypeError)):
            with pytest.raises(err):
                call(ok, after=after)
    lim, flags, cur = vrod_amd.Index._order_args(7, True, (I64_MIN, (1 << 64) - 1), True)
    assert (lim, flags) == (7, 3) and cur.dtype == vrod_amd.ORDER_CURSOR_DTYPE and cur.tolist() == [(I64_MIN, (1 << 64) - 1)]
    assert cur.view(np.uint64).tolist() == [1 << 63, (1 << 64) - 1]              # the bytes the library reads
    assert vrod_amd.Index._order_args(0, False, None, False) == (0, 0, None)
    assert vrod_amd.Index._order_args(np.int64(65536), np.bool_(False), [np.int64(-1), np.uint64(3)], False)[2].tolist() == [(-1, 3)]
    assert vrod_amd.Index._order_args(1, False, cur[0], False)[2].tolist() == cur.tolist()   # one element of a cursor array
