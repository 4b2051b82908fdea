"""CPU tests of the duplicate-row entry points (vrod_index_find_duplicates, _find_duplicates_device, _delete_duplicates):
the three names in every layer, the stats struct's layout, argument validation that needs no device, the Python wrappers'
own checks, and the model (dup_model) on hand-made arrays."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dup_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u32, u64, pu64 = C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)
NAMES = ["vrod_index_find_duplicates", "vrod_index_find_duplicates_device", "vrod_index_delete_duplicates"]
FIELDS = ["live", "classes", "duplicates", "largest_class", "slots", "max_probe", "compare_misses"]
NONE = int(dup_model.ID_NONE)


def test_names_in_every_layer():
    import vrod_amd
    from vrod_amd._lib import DupStats
    L = vrod_amd.load()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ps = C.POINTER(DupStats)
    argtypes = {NAMES[0]: [vp, u32, vp, u64, ps], NAMES[1]: [vp, u32, vp, u64, ps, vp], NAMES[2]: [vp, u32, pu64]}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in vrod.h"
        assert name in vrod_amd.SYMBOLS and hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == argtypes[name], name
        assert getattr(L, name).restype in (C.c_int, C.c_int32), name
        assert re.search(r"\bpub fn %s\s*\(" % name, rust), f"{name} is not in the Rust binding"
    assert [f for f, _ in DupStats._fields_] == FIELDS and C.sizeof(DupStats) == 56
    assert re.search(r"typedef struct\s*\{\s*" + r"[^}]*".join(r"uint64_t\s+%s;" % f for f in FIELDS) + r"[^}]*\}\s*vrod_dup_stats;", header)
    assert re.search(r"pub struct vrod_dup_stats\s*\{\s*" + r"\s*".join(r"pub %s: u64," % f for f in FIELDS) + r"\s*\}", rust)
    assert re.search(r"#define VROD_DUP_WITHIN_LABEL 1u", header) and re.search(r"#define VROD_DUP_NARROW_HASH\s+0x80000000u", header)
    assert re.search(r"pub const VROD_DUP_WITHIN_LABEL: u32 = 1;", rust) and re.search(r"pub const VROD_DUP_NARROW_HASH: u32 = 0x8000_0000;", rust)
    assert (vrod_amd.DUP_WITHIN_LABEL, vrod_amd.DUP_NARROW_HASH) == (dup_model.DUP_WITHIN_LABEL, dup_model.DUP_NARROW_HASH) == (1, 0x80000000)
    for method in ("find_duplicates", "find_duplicates_device", "delete_duplicates"):
        assert callable(getattr(vrod_amd.Index, method))
    section = header[header.index("/* Duplicate rows"):header.index("#define VROD_DUP_WITHIN_LABEL")]
    assert "SMALLEST ID" in section and "DIAGNOSTICS" in section and "diagnostic" in section   # the survivor rule and the diagnostics are stated
    assert "dup_plan.h" in open(os.path.join(ROOT, "vrod_amd", "csrc", "Makefile")).read()
    assert "kernels_dup.hip" in open(os.path.join(ROOT, "vrod_amd", "csrc", "Makefile")).read()


def test_stats_struct_is_seven_words(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_dup_stats) == 56, "vrod_dup_stats");\n'
                   + "".join('_Static_assert(offsetof(vrod_dup_stats, %s) == %d, "%s");\n' % (f, 8 * i, f) for i, f in enumerate(FIELDS))
                   + '_Static_assert(VROD_DUP_WITHIN_LABEL == 1u && VROD_DUP_NARROW_HASH == 0x80000000u, "flags");\n'
                   'int main(void) { vrod_dup_stats s = {0}; return (int)s.live; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)


def test_argument_validation_without_device():
    """A null handle is refused by every entry point whatever else it is given, and no output is written."""
    import vrod_amd
    from vrod_amd._lib import DupStats
    L = vrod_amd.load()
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    st = DupStats(*([9] * 7))
    n = C.c_uint64(7)
    for flags in (0, 1, 2, 0x80000000, 0x80000001, 0xFFFFFFFF):
        for map_len in (0, 4):
            assert L.vrod_index_find_duplicates(None, flags, out, map_len, C.byref(st)) == 1
            assert L.vrod_index_find_duplicates(None, flags, None, map_len, None) == 1
            assert L.vrod_index_find_duplicates_device(None, flags, out, map_len, C.byref(st), None) == 1
        assert L.vrod_index_delete_duplicates(None, flags, C.byref(n)) == 1
        assert L.vrod_index_delete_duplicates(None, flags, None) == 1
    assert list(out) == [7, 7, 7, 7] and n.value == 7 and all(getattr(st, f) == 9 for f in FIELDS)
    assert L.vrod_last_error()


def test_wrappers_check_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, None, 0
    for call in (lambda: ix.find_duplicates(within_label=1), lambda: ix.find_duplicates(narrow_hash="yes"), lambda: ix.find_duplicates_device(within_label=None),
                 lambda: ix.delete_duplicates(within_label=0)):
        with pytest.raises(TypeError):
            call()
    assert vrod_amd.Index._dup_flags(True, True) == 0x80000001 and vrod_amd.Index._dup_flags(False) == 0
    assert vrod_amd.Index._dup_flags(np.bool_(True)) == 1


# ---------------------------------------------------------------- the model on hand-made arrays
def test_model_groups_by_bits():
    a = np.array([1.0, 2.0, 0.0, -3.5], np.float32)
    rows = np.stack([a, a + 1, a, a, a + 1, a])                                  # classes {0, 2, 3, 5} and {1, 4}
    out, st = dup_model.find_duplicates(rows)
    assert out.dtype == np.uint64 and out.tolist() == [0, 1, 0, 0, 1, 0]
    assert st == {"live": 6, "classes": 2, "duplicates": 4, "largest_class": 4}
    out, st = dup_model.find_duplicates(rows, id_offset=5000)
    assert out.tolist() == [5000, 5001, 5000, 5000, 5001, 5000]
    # the smallest id of a class is deleted: the next live one is the first; all but one deleted: it is its own first
    out, st = dup_model.find_duplicates(rows, deleted=[0, 1])
    assert out.tolist() == [NONE, NONE, 2, 2, 4, 2] and st == {"live": 4, "classes": 2, "duplicates": 2, "largest_class": 3}
    out, st = dup_model.find_duplicates(rows, deleted=range(6))
    assert out.tolist() == [NONE] * 6 and st == {"live": 0, "classes": 0, "duplicates": 0, "largest_class": 0}
    out, st = dup_model.find_duplicates(np.zeros((0, 4), np.float32))
    assert out.size == 0 and st["largest_class"] == 0 and st["live"] == 0


def test_model_tells_near_copies_apart():
    a = np.array([1.0, 2.0, 0.0, -3.5, 7.0], np.float32)
    last, first, sign, swap = a.copy(), a.copy(), a.copy(), a.copy()
    last[-1], first[0], sign[2] = np.nextafter(a[-1], np.float32(np.inf)), np.nextafter(a[0], np.float32(0)), -0.0
    swap[[1, 3]] = a[[3, 1]]
    assert a[2] == sign[2] and np.signbit(sign[2])                               # equal as numbers, different bits
    out, st = dup_model.find_duplicates(np.stack([a, last, first, sign, swap, a]))
    assert out.tolist() == [0, 1, 2, 3, 4, 0] and st["classes"] == 5 and st["largest_class"] == 2
    nan = a.copy()
    nan[0] = np.nan
    out, _ = dup_model.find_duplicates(np.stack([nan, nan]))                     # bits, not comparisons: a NaN equals itself
    assert out.tolist() == [0, 0]


def test_model_within_label():
    a = np.ones(3, np.float32)
    rows = np.stack([a, a, a, a, 2 * a])
    labels = np.array([7, 9, 7, 9, 7], np.uint32)
    out, st = dup_model.find_duplicates(rows, labels=labels, within_label=True)
    assert out.tolist() == [0, 1, 0, 1, 4] and dup_model.exact(st) == {"live": 5, "classes": 3, "duplicates": 2, "largest_class": 2}
    out, st = dup_model.find_duplicates(rows, labels=labels, within_label=False)   # without the flag the labels are not read
    assert out.tolist() == [0, 0, 0, 0, 4] and st["largest_class"] == 4
    out, st = dup_model.find_duplicates(rows, labels=None, within_label=True)      # no labels: label 0 everywhere
    assert out.tolist() == [0, 0, 0, 0, 4]
