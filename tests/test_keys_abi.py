"""CPU tests of the row-key entry points (vrod_index_set_keys, _get_keys, _find_keys, _find_keys_device, _ids_to_keys,
_ids_to_keys_device, _delete_keys, _upsert, _key_stats): the nine names in every layer, the stats struct's layout, the
argument validation that needs no device, the Python wrappers' own checks and the plain-Python model the GPU tests compare
against (keys_model.KeysModel), on its own."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from index_model import ERR_INVALID_ARG, ERR_INVALID_VALUE, ModelError
from keys_model import KeysModel, NONE
from support import ID_NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64 = C.c_void_p, C.c_uint64
ARGTYPES = {
    "vrod_index_set_keys": [vp, u64, vp, u64],
    "vrod_index_get_keys": [vp, u64, u64, vp],
    "vrod_index_find_keys": [vp, vp, u64, vp],
    "vrod_index_find_keys_device": [vp, vp, u64, vp, vp],
    "vrod_index_ids_to_keys": [vp, vp, u64, vp],
    "vrod_index_ids_to_keys_device": [vp, vp, u64, vp, vp],
    "vrod_index_delete_keys": [vp, vp, u64, C.POINTER(u64)],
    "vrod_index_upsert": [vp, vp, vp, u64, vp],
}
STATS_FIELDS = ["keyed_live", "slots", "occupied", "rebuilds", "max_probe"]


def test_names_in_every_layer():
    import vrod_amd
    from vrod_amd._lib import KeyStats
    L = vrod_amd.load()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in list(ARGTYPES) + ["vrod_index_key_stats"]:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in vrod.h"
        assert name in vrod_amd.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported"
        assert getattr(L, name).restype in (C.c_int, C.c_int32), name
        assert re.search(r"\bpub fn %s\s*\(" % name, rust), f"{name} is not in the Rust binding"
    for name, types in ARGTYPES.items():
        assert list(getattr(L, name).argtypes) == types, name
    assert list(L.vrod_index_key_stats.argtypes) == [vp, C.POINTER(KeyStats)]
    assert [f for f, _ in KeyStats._fields_] == STATS_FIELDS and C.sizeof(KeyStats) == 40
    assert re.search(r"pub struct vrod_key_stats\s*\{\s*" + r"\s*".join(rf"pub {f}: u64," for f in STATS_FIELDS) + r"\s*\}", rust)
    for method in ("set_keys", "get_keys", "find_keys", "find_keys_device", "ids_to_keys", "ids_to_keys_device", "delete_keys", "upsert",
                   "key_stats"):
        assert callable(getattr(vrod_amd.Index, method)), method
    info = re.search(r"struct vrod_snapshot_info \{[^}]*\}", header).group(0)
    assert "has_values" in info and "has_keys" not in info                      # the info struct keeps its layout


def test_stats_struct_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    checks = "".join(f'_Static_assert(offsetof(vrod_key_stats, {f}) == {8 * i}, "{f}");\n' for i, f in enumerate(STATS_FIELDS))
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_key_stats) == 40, "vrod_key_stats");\n' + checks +
                   'int main(void) { return VROD_ID_NONE == UINT64_MAX ? 0 : 1; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)


def test_argument_validation_without_device():
    import vrod_amd
    from vrod_amd._lib import KeyStats
    L = vrod_amd.load()
    a, b = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    rows = (C.c_float * 32)()
    died = C.c_uint64(7)
    st = KeyStats()
    for n in (4, 0):                                                             # a null handle is refused whatever n is
        assert L.vrod_index_set_keys(None, 0, a, n) == 1
        assert L.vrod_index_get_keys(None, 0, n, a) == 1
        assert L.vrod_index_find_keys(None, a, n, b) == 1
        assert L.vrod_index_find_keys_device(None, a, n, b, None) == 1
        assert L.vrod_index_ids_to_keys(None, a, n, b) == 1
        assert L.vrod_index_ids_to_keys_device(None, a, n, b, None) == 1
        assert L.vrod_index_delete_keys(None, a, n, C.byref(died)) == 1
        assert L.vrod_index_upsert(None, a, rows, n, b) == 1
    assert died.value == 0                                                       # (written before anything is looked at)
    assert L.vrod_index_set_keys(None, 0, None, 4) == 1                          # null pointers with a null handle
    assert L.vrod_index_find_keys(None, None, 4, None) == 1
    assert L.vrod_index_ids_to_keys(None, None, 4, None) == 1
    assert L.vrod_index_delete_keys(None, None, 4, None) == 1
    assert L.vrod_index_upsert(None, None, None, 4, None) == 1
    assert L.vrod_index_key_stats(None, C.byref(st)) == 1
    assert L.vrod_index_key_stats(None, None) == 1
    assert b"null" in L.vrod_last_error()


def test_python_wrappers_check_their_arguments():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)                                  # no device: a wrapper over a null handle
    ix._L, ix._h, ix.dim = vrod_amd.load(), None, 8
    with pytest.raises(TypeError):
        ix.set_keys(0, np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        ix.set_keys(0, [-1, 2])
    with pytest.raises(TypeError):
        ix.find_keys(["a"])
    with pytest.raises(ValueError):
        ix.upsert([1, 2], np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError):
        ix.upsert([1, 2], np.zeros((2, 7), np.float32))
    for call in (lambda: ix.set_keys(0, [1, 2]), lambda: ix.get_keys(0, 2), lambda: ix.find_keys([1, NONE]), lambda: ix.ids_to_keys([[0, 1]]),
                 lambda: ix.delete_keys([1]), lambda: ix.upsert([1, 2], np.zeros((2, 8), np.float32)), ix.key_stats):
        with pytest.raises(vrod_amd.VrodError) as e:
            call()
        assert e.value.code == 1
    ix._h = None                                                                 # (nothing for __del__ to destroy)


def test_the_model_on_its_own():
    rng = np.random.default_rng(5)
    m = KeysModel(8, "f32", "l2", id_offset=100)
    m.add(rng.standard_normal((6, 8)).astype(np.float32))
    assert np.array_equal(m.get_keys(100, 6), np.full(6, ID_NONE)) and m.keyed_live() == 0
    m.set_keys(101, [11, 12, 13])
    assert np.array_equal(m.find_keys([12, 11, 99, NONE, 12]), np.array([102, 101, NONE, NONE, 102], np.uint64))
    for first, keys in ((100, [12]), (104, [5, 5]), (105, [1, 2]), (99, [1])):   # held outside, twice, past the rows, below the offset
        with pytest.raises(ModelError) as e:
            m.set_keys(first, keys)
        assert e.value.code == ERR_INVALID_ARG
    m.set_keys(101, [13, 11, 12])                                                # a permutation
    m.set_keys(104, [NONE, NONE])                                                # no key may repeat
    m.delete([102])
    assert m.find_keys([11])[0] == ID_NONE and m.get_keys(102, 1)[0] == 11 and m.keyed_live() == 2
    m.set_keys(100, [11])                                                        # a deleted row's key is free
    m.set_keys(102, [11])                                                        # ... and a deleted row may carry a live row's key
    assert m.find_keys([11])[0] == 100
    assert np.array_equal(m.ids_to_keys([[102, 100], [NONE, 106]]), np.array([[11, 11], [NONE, NONE]], np.uint64))
    ids = m.upsert([13, 77, 12, 78], rng.standard_normal((4, 8)).astype(np.float32))
    assert np.array_equal(ids, np.array([101, 106, 103, 107], np.uint64)) and m.count == 8
    for keys, raw, code in (([1, 1], np.zeros((2, 8)), ERR_INVALID_ARG), ([NONE], np.zeros((1, 8)), ERR_INVALID_ARG),
                            ([5], np.full((1, 8), np.nan), ERR_INVALID_VALUE)):
        with pytest.raises(ModelError) as e:
            m.upsert(keys, raw)
        assert e.value.code == code and m.count == 8
    assert m.delete_keys([77, 77, 4242, 11]) == 2 and m.live_count() == 5
    new_ids = m.compact()
    assert m.count == 5 and np.array_equal(m.find_keys([13, 12, 78]), new_ids[[1, 3, 7]]) and m.find_keys([77])[0] == ID_NONE
