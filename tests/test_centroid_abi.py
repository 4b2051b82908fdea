"""CPU tests of the group-centroid entry points (vrod_index_centroids_where, _device): the names in every layer, the group
struct's size and offsets, the constants, argument validation that needs no device, and the Python wrapper's own checks."""
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
NAMES = {"vrod_index_centroids_where": [vp, vp, u32, u32, C.c_int64, u32, pu64, pu64, vp, vp, u64],
         "vrod_index_centroids_where_device": [vp, vp, u32, u32, C.c_int64, u32, pu64, pu64, vp, vp, u64, vp]}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FIELDS = [("key", np.int64, 0), ("count", np.uint64, 8), ("first_id", np.uint64, 16)]
CONSTANTS = {"VROD_CENTROID_SUM": 8, "VROD_MAX_CENTROID_GROUPS": 65536}


def test_names_in_every_layer():
    import vrod_amd
    L = vrod_amd.load()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, argtypes in NAMES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in vrod.h"
        assert name in vrod_amd.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported"
        assert list(getattr(L, name).argtypes) == argtypes
        assert getattr(L, name).restype in (C.c_int, C.c_int32)
        assert re.search(r"\bpub fn %s\s*\(" % name, rust), f"{name} is not in the Rust binding"
    assert re.search(r"typedef struct\s*\{\s*int64_t\s+key;\s*uint64_t\s+count;[^}]*uint64_t\s+first_id;[^}]*\}\s*vrod_centroid_group;", header)
    assert re.search(r"#\[repr\(C\)\][^{}]*pub struct vrod_centroid_group\s*\{\s*pub key: i64,\s*pub count: u64,\s*pub first_id: u64,\s*\}", rust)
    assert callable(vrod_amd.Index.centroids_where)
    makefile = open(os.path.join(ROOT, "vrod_amd", "csrc", "Makefile")).read()
    assert "kernels_centroid.hip" in makefile and "centroid_plan.h" in makefile


def test_the_constants_in_every_layer():
    import vrod_amd
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, value in CONSTANTS.items():
        assert re.search(r"#define %s\s+%du\b" % (name, value), header), name
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rust), name
        assert getattr(vrod_amd, name[len("VROD_"):]) == value
    # the flags word is shared: ALLOWED is 1, ORDER_DESC 2 and AGG_ORDER_COUNT 4 are not flags of this call
    assert vrod_amd.CENTROID_SUM & (vrod_amd.ROWPRED_ALLOWED | vrod_amd.ORDER_DESC | vrod_amd.AGG_ORDER_COUNT) == 0
    assert vrod_amd.MAX_CENTROID_GROUPS <= vrod_amd.MAX_AGG_GROUPS


def test_group_struct_is_24_bytes(tmp_path):
    import vrod_amd
    DT = vrod_amd.CENTROID_GROUP_DTYPE
    assert DT.itemsize == 24 and DT.names == tuple(f[0] for f in FIELDS)
    assert [(n, DT[n], DT.fields[n][1]) for n in DT.names] == [(n, np.dtype(t), o) for n, t, o in FIELDS]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_centroid_group) == 24, "vrod_centroid_group");\n'
                   + "".join('_Static_assert(offsetof(vrod_centroid_group, %s) == %d, "%s");\n' % (n, o, n) for n, _, o in FIELDS)
                   + '_Static_assert(VROD_CENTROID_SUM == 8 && VROD_MAX_CENTROID_GROUPS == 65536, "the constants");\n'
                   '_Static_assert((VROD_CENTROID_SUM & (VROD_ROWPRED_ALLOWED | VROD_ORDER_DESC | VROD_AGG_ORDER_COUNT)) == 0, "the flags word is shared");\n'
                   'int main(void) { vrod_centroid_group g = {-1, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull};\n'
                   '    /* the prototypes, in an operand that is not evaluated: nothing to link */\n'
                   '    (void)sizeof(vrod_index_centroids_where((vrod_index *)0, (const vrod_row_pred *)0, 0u, 0u, (int64_t)0, 0u, (uint64_t *)0, (uint64_t *)0,\n'
                   '                                            &g, (float *)0, (uint64_t)0));\n'
                   '    (void)sizeof(vrod_index_centroids_where_device((vrod_index *)0, (const vrod_row_pred *)0, 0u, 0u, (int64_t)0, 0u, (uint64_t *)0,\n'
                   '                                                   (uint64_t *)0, &g, (float *)0, (uint64_t)0, (void *)0));\n'
                   '    return g.key < 0 && g.count > 0 && g.first_id > 0 ? 0 : 1; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)                         # the key is signed, count and id are not


def test_argument_validation_without_device():
    """A null handle is refused for every combination of the other arguments, and nothing is written."""
    import vrod_amd
    L = vrod_amd.load()
    good = np.zeros(1, vrod_amd.ROWPRED_DTYPE)
    good["lo"], good["hi"] = I64_MIN, I64_MAX
    bad_label = good.copy()
    bad_label["has_label"] = 2
    groups = np.full(4, 7, vrod_amd.CENTROID_GROUP_DTYPE)
    vectors = np.full((4, 8), 7.0, np.float32)
    n, rows = C.c_uint64(7), C.c_uint64(7)
    preds = [p.ctypes.data_as(vp) for p in (good, bad_label)] + [None]
    combos = itertools.product(preds, (0, 1, 2, 4, 8, 9, 0xFFFFFFFF), (0, 1, 2, 0xFFFFFFFF), (I64_MIN, 0, 1, I64_MAX), (0, 4, 65536, 65537, 0xFFFFFFFF),
                               (None, C.byref(n)), (None, C.byref(rows)), (None, groups.ctypes.data_as(vp)), (None, vectors.ctypes.data_as(vp)),
                               (0, 7, 8, (1 << 64) - 1))
    seen = 0
    for pp, flags, by, width, capacity, pn, pr, pg, pv, stride in combos:
        assert L.vrod_index_centroids_where(None, pp, flags, by, width, capacity, pn, pr, pg, pv, stride) == 1
        assert L.vrod_index_centroids_where_device(None, pp, flags, by, width, capacity, pn, pr, pg, pv, stride, None) == 1
        seen += 1
    assert seen == 3 * 7 * 4 * 4 * 5 * 16 * 4
    assert (groups.view(np.uint64) == np.full(4, 7, vrod_amd.CENTROID_GROUP_DTYPE).view(np.uint64)).all() and (vectors == 7.0).all()
    assert (n.value, rows.value) == (7, 7)
    assert L.vrod_last_error()


def test_wrapper_checks_before_the_library():
    import vrod_amd
    va = vrod_amd
    ix = va.Index.__new__(va.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, None, 0
    ok = va.Index.row_pred()
    with pytest.raises(ValueError):
        ix.centroids_where([[0, 0, 0, 0, 0, 0, 2]], va.AGG_BY_LABEL, capacity=4)     # has_label
    with pytest.raises(TypeError):
        ix.centroids_where(np.zeros((1, 7), np.float64), va.AGG_BY_LABEL, capacity=4)
    with pytest.raises(ValueError):
        ix.centroids_where(np.concatenate([ok, ok]), va.AGG_BY_LABEL, capacity=4)    # one predicate per call
    for by, err in ((va.AGG_BY_TAG, ValueError), (3, ValueError), (-1, ValueError), ("label", TypeError), (1.0, TypeError), (True, TypeError), (None, TypeError)):
        with pytest.raises(err):
            ix.centroids_where(ok, by, width=5, capacity=4)
    for width, err in ((0, ValueError), (-1, ValueError), (1 << 63, ValueError), (None, ValueError), (2.0, TypeError), (True, TypeError)):
        with pytest.raises(err):
            ix.centroids_where(ok, va.AGG_BY_VALUE, width=width, capacity=4)
    for capacity, err in ((0, ValueError), (-1, ValueError), (va.MAX_CENTROID_GROUPS + 1, ValueError), (2.0, TypeError), ("5", TypeError), (True, TypeError)):
        with pytest.raises(err, match="capacity"):                                # the message names this method's argument
            ix.centroids_where(ok, va.AGG_BY_LABEL, capacity=capacity)
    with pytest.raises(TypeError):
        ix.centroids_where(ok, va.AGG_BY_LABEL, capacity=4, sums=1)
    with pytest.raises(TypeError):
        ix.centroids_where(ok, va.AGG_BY_LABEL, capacity=4, allowed_only="yes")
    with pytest.raises(ValueError):
        ix.centroids_where(ok, va.AGG_BY_LABEL, capacity=4, out=np.zeros((4, 4), np.float32))   # not a torch tensor
