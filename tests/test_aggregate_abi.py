"""CPU tests of the row-aggregation entry point (vrod_index_aggregate_where): the name in every layer, the group struct's
size and offsets, the five constants, argument validation that needs no device, and the Python wrapper's own checks."""
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
NAME = "vrod_index_aggregate_where"
ARGTYPES = [vp, vp, u32, u32, C.c_int64, u32, pu64, pu64, pu64, vp]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FIELDS = [("key", np.int64, 0), ("count", np.uint64, 8), ("min_value", np.int64, 16), ("max_value", np.int64, 24), ("sum_value", np.int64, 32),
          ("first_id", np.uint64, 40)]
CONSTANTS = {"VROD_AGG_BY_LABEL": 0, "VROD_AGG_BY_VALUE": 1, "VROD_AGG_BY_TAG": 2, "VROD_AGG_ORDER_COUNT": 4, "VROD_MAX_AGG_GROUPS": 1048576}


def test_name_in_every_layer():
    import vrod_amd
    L = vrod_amd.load()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header), f"{NAME} is not declared in vrod.h"
    assert NAME in vrod_amd.SYMBOLS
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert list(getattr(L, NAME).argtypes) == ARGTYPES
    assert getattr(L, NAME).restype in (C.c_int, C.c_int32)
    assert re.search(r"\bpub fn %s\s*\(" % NAME, rust), f"{NAME} is not in the Rust binding"
    assert re.search(r"typedef struct\s*\{\s*int64_t\s+key;\s*uint64_t\s+count;[^}]*int64_t\s+min_value, max_value;\s*int64_t\s+sum_value;[^}]*"
                     r"uint64_t\s+first_id;[^}]*\}\s*vrod_agg_group;", header)
    assert re.search(r"#\[repr\(C\)\][^{}]*pub struct vrod_agg_group\s*\{\s*pub key: i64,\s*pub count: u64,\s*pub min_value: i64,\s*pub max_value: i64,\s*"
                     r"pub sum_value: i64,\s*pub first_id: u64,\s*\}", rust)
    assert callable(vrod_amd.Index.aggregate_where)


def test_the_constants_in_every_layer():
    import vrod_amd
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, value in CONSTANTS.items():
        assert re.search(r"#define %s\s+%du\b" % (name, value), header), name
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rust), name
        assert getattr(vrod_amd, name[len("VROD_"):]) == value
    # the flags word is shared: ALLOWED is 1, ORDER_DESC stays 2 and is not a flag of this call
    assert vrod_amd.AGG_ORDER_COUNT & (vrod_amd.ROWPRED_ALLOWED | vrod_amd.ORDER_DESC) == 0


def test_group_struct_is_48_bytes(tmp_path):
    import vrod_amd
    DT = vrod_amd.AGG_GROUP_DTYPE
    assert DT.itemsize == 48 and DT.names == tuple(f[0] for f in FIELDS)
    assert [(n, DT[n], DT.fields[n][1]) for n in DT.names] == [(n, np.dtype(t), o) for n, t, o in FIELDS]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_agg_group) == 48, "vrod_agg_group");\n'
                   + "".join('_Static_assert(offsetof(vrod_agg_group, %s) == %d, "%s");\n' % (n, o, n) for n, _, o in FIELDS)
                   + '_Static_assert(VROD_AGG_BY_LABEL == 0 && VROD_AGG_BY_VALUE == 1 && VROD_AGG_BY_TAG == 2 && VROD_AGG_ORDER_COUNT == 4 && '
                   'VROD_MAX_AGG_GROUPS == 1048576, "the constants");\n'
                   '_Static_assert((VROD_AGG_ORDER_COUNT & (VROD_ROWPRED_ALLOWED | VROD_ORDER_DESC)) == 0, "the flags word is shared");\n'
                   'int main(void) { vrod_agg_group g = {-1, 0xFFFFFFFFFFFFFFFFull, -1, -1, -1, 0xFFFFFFFFFFFFFFFFull};\n'
                   '    return g.key < 0 && g.count > 0 && g.min_value < 0 && g.max_value < 0 && g.sum_value < 0 && g.first_id > 0 ? 0 : 1; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)                         # key and values are signed, count and id are not


def test_argument_validation_without_device():
    """A null handle is refused for every combination of the other arguments, and nothing is written."""
    import vrod_amd
    L = vrod_amd.load()
    good = np.zeros(1, vrod_amd.ROWPRED_DTYPE)
    good["lo"], good["hi"] = I64_MIN, I64_MAX
    bad_label = good.copy()
    bad_label["has_label"] = 2
    out = np.full(4, 7, vrod_amd.AGG_GROUP_DTYPE)
    n, groups, rows = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    preds = [p.ctypes.data_as(vp) for p in (good, bad_label)] + [None]
    combos = itertools.product(preds, (0, 1, 2, 4, 5, 8, 0xFFFFFFFF), (0, 1, 2, 3, 0xFFFFFFFF), (I64_MIN, -1, 0, 1, I64_MAX), (0, 4, 1 << 20, 0xFFFFFFFF),
                               (None, C.byref(n)), (None, C.byref(groups)), (None, C.byref(rows)), (None, out.ctypes.data_as(vp)))
    seen = 0
    for pp, flags, by, width, limit, pn, pg, pr, po in combos:
        assert L.vrod_index_aggregate_where(None, pp, flags, by, width, limit, pn, pg, pr, po) == 1
        seen += 1
    assert seen == 3 * 7 * 5 * 5 * 4 * 16
    assert (out.view(np.uint64) == np.full(4, 7, vrod_amd.AGG_GROUP_DTYPE).view(np.uint64)).all() and (n.value, groups.value, rows.value) == (7, 7, 7)
    assert L.vrod_last_error()


def test_wrapper_checks_before_the_library():
    import vrod_amd
    va = vrod_amd
    ix = va.Index.__new__(va.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, None, 0
    ok = va.Index.row_pred()
    with pytest.raises(ValueError):
        ix.aggregate_where([[0, 0, 0, 0, 0, 0, 2]], va.AGG_BY_LABEL)             # has_label
    with pytest.raises(TypeError):
        ix.aggregate_where(np.zeros((1, 7), np.float64), va.AGG_BY_LABEL)
    with pytest.raises(ValueError):
        ix.aggregate_where(np.concatenate([ok, ok]), va.AGG_BY_LABEL)            # one predicate per call
    for by, err in ((3, ValueError), (-1, ValueError), (1 << 40, ValueError), ("label", TypeError), (1.0, TypeError), (True, TypeError), (None, TypeError)):
        with pytest.raises(err):
            ix.aggregate_where(ok, by, width=5)
    for width, err in ((0, ValueError), (-1, ValueError), (1 << 63, ValueError), (None, ValueError), (2.0, TypeError), ("7", TypeError), (True, TypeError)):
        with pytest.raises(err):
            ix.aggregate_where(ok, va.AGG_BY_VALUE, width=width)
    for width, err in ((0, ValueError), (2.0, TypeError)):                        # checked in the other modes too, where the library does not read it
        with pytest.raises(err):
            ix.aggregate_where(ok, va.AGG_BY_TAG, width=width)
    for limit, err in ((-1, ValueError), (1 << 32, ValueError), (2.0, TypeError), ("5", TypeError), (True, TypeError)):
        with pytest.raises(err):
            ix.aggregate_where(ok, va.AGG_BY_LABEL, limit=limit)
    with pytest.raises(TypeError):
        ix.aggregate_where(ok, va.AGG_BY_LABEL, by_count=1)
    with pytest.raises(TypeError):
        ix.aggregate_where(ok, va.AGG_BY_LABEL, allowed_only="yes")
    A = va.Index._agg_args
    assert A(va.AGG_BY_LABEL, None, None, False, False) == (0, 0, None, 0)
    assert A(va.AGG_BY_VALUE, I64_MAX, 0, True, True) == (1, I64_MAX, 0, 5)
    assert A(np.uint32(2), np.int64(9), np.int64((1 << 32) - 1), np.bool_(True), np.bool_(False)) == (2, 0, (1 << 32) - 1, 4)   # width unread under BY_TAG
