"""CPU tests of the row-tag entry points (vrod_index_set_tags, vrod_index_get_tags, vrod_search_tagged,
vrod_search_tagged_device): the four names in every layer, the predicate struct's size, argument validation that needs no
device, and the Python wrappers' own checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vrod_index_set_tags", "vrod_index_get_tags", "vrod_search_tagged", "vrod_search_tagged_device"]
vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
ARGTYPES = {
    "vrod_index_set_tags": [vp, u64, vp, u64],
    "vrod_index_get_tags": [vp, u64, u64, vp],
    "vrod_search_tagged": [vp, vp, u32, u32, vp, vp, vp],
    "vrod_search_tagged_device": [vp, vp, u32, u32, vp, vp, vp, vp],
}


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
    assert re.search(r"typedef struct\s*\{\s*uint64_t any, all, none;\s*\}\s*vrod_tag_pred;", header)
    assert re.search(r"#\[repr\(C\)\][^{}]*pub struct vrod_tag_pred\s*\{\s*pub any: u64,\s*pub all: u64,\s*pub none: u64,\s*\}", rust)


def test_predicate_struct_is_24_bytes(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include "vrod.h"\n_Static_assert(sizeof(vrod_tag_pred) == 24, "vrod_tag_pred"); int main(void) { return 0; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)


def test_tag_argument_validation_without_device():
    import vrod_amd
    L = vrod_amd.load()
    buf = (C.c_uint64 * 4)()
    preds = (C.c_uint64 * 3)()
    q = (C.c_float * 4)()
    ids = (C.c_uint64 * 4)()
    sc = (C.c_float * 4)()
    assert L.vrod_index_set_tags(None, 0, buf, 4) == 1
    assert L.vrod_index_set_tags(None, 0, None, 0) == 1
    assert L.vrod_index_get_tags(None, 0, 4, buf) == 1
    assert L.vrod_index_get_tags(None, 0, 0, None) == 1
    assert L.vrod_search_tagged(None, q, 1, 1, preds, ids, sc) == 1
    assert L.vrod_search_tagged(None, None, 1, 1, None, None, None) == 1
    assert L.vrod_search_tagged_device(None, q, 1, 1, preds, ids, sc, None) == 1
    assert L.vrod_search_tagged_device(None, None, 1, 1, None, None, None, None) == 1
    assert L.vrod_last_error()


def test_wrappers_reject_bad_tag_arrays():
    import vrod_amd
    f = vrod_amd.Index._u64
    with pytest.raises(TypeError):
        f(np.zeros(4, np.float32), "tags", (-1,))
    with pytest.raises(TypeError):
        f(np.zeros(4, bool), "tags", (-1,))
    with pytest.raises(ValueError):
        f(np.array([-1, 2]), "tags", (-1,))
    with pytest.raises(ValueError):
        f(np.zeros((4, 2), np.uint64), "preds", (4, 3))
    a = f(np.array([[1, 2], [3, 1 << 40]], np.int64), "tags", (-1,))
    assert a.dtype == np.uint64 and a.tolist() == [1, 2, 3, 1 << 40] and a.flags.c_contiguous
    top = f([1 << 63, 0xFFFFFFFFFFFFFFFF], "tags", (-1,))
    assert top.dtype == np.uint64 and top.tolist() == [1 << 63, 0xFFFFFFFFFFFFFFFF]          # bit 63 survives
    assert f([], "tags", (-1,)).size == 0 and f([], "tags", (-1,)).dtype == np.uint64
    p = f(np.arange(6, dtype=np.uint64)[::-1].reshape(2, 3), "preds", (2, 3))
    assert p.flags.c_contiguous and p.tolist() == [[5, 4, 3], [2, 1, 0]]


def test_search_tagged_checks_predicates_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    q = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError):
        ix.search_tagged(q, 2, np.zeros((2, 3), np.uint64))
    with pytest.raises(ValueError):
        ix.search_tagged(q, 2, np.zeros(3, np.uint64))
    with pytest.raises(TypeError):
        ix.search_tagged(q, 2, np.zeros((3, 3), np.float64))
