"""CPU tests of the near-duplicate entry points (vrod_index_find_near_duplicates, _find_near_duplicates_device,
_delete_near_duplicates): the three names in every layer, the stats struct's layout, the flag's value, argument
validation that needs no device, and the Python wrappers' own checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import near_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u32, u64, f32, pu64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.POINTER(C.c_uint64)
NAMES = ["vrod_index_find_near_duplicates", "vrod_index_find_near_duplicates_device", "vrod_index_delete_near_duplicates"]
FIELDS = ["rows", "classes", "near_duplicates", "largest_class", "hits", "batches", "splits", "pool_entries"]


def test_names_in_every_layer():
    import vrod_amd
    from vrod_amd._lib import NearStats
    L = vrod_amd.load()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ps = C.POINTER(NearStats)
    argtypes = {NAMES[0]: [vp, f32, u32, vp, u64, ps], NAMES[1]: [vp, f32, u32, vp, u64, ps, vp], NAMES[2]: [vp, f32, u32, pu64]}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in vrod.h"
        assert name in vrod_amd.SYMBOLS and hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == argtypes[name], name
        assert getattr(L, name).restype in (C.c_int, C.c_int32), name
        assert re.search(r"\bpub fn %s\s*\(" % name, rust), f"{name} is not in the Rust binding"
    assert [f for f, _ in NearStats._fields_] == FIELDS and C.sizeof(NearStats) == 64
    assert re.search(r"typedef struct\s*\{\s*" + r"[^}]*".join(r"uint64_t\s+%s;" % f for f in FIELDS) + r"[^}]*\}\s*vrod_near_stats;", header)
    assert re.search(r"pub struct vrod_near_stats\s*\{\s*" + r"\s*".join(r"pub %s: u64," % f for f in FIELDS) + r"\s*\}", rust)
    assert re.search(r"#define VROD_NEAR_SMALL_POOL 0x80000000u", header)
    assert re.search(r"pub const VROD_NEAR_SMALL_POOL: u32 = 0x8000_0000;", rust)
    assert vrod_amd.NEAR_SMALL_POOL == near_model.NEAR_SMALL_POOL == 0x80000000
    for method in ("find_near_duplicates", "find_near_duplicates_device", "delete_near_duplicates"):
        assert callable(getattr(vrod_amd.Index, method))
    section = header[header.index("/* Near-duplicate rows"):header.index("#define VROD_NEAR_SMALL_POOL")]
    for said in ("SMALLEST ID", "DIAGNOSTICS", "CHAINING", "SINGLE LINKAGE", "IGNORES THE FILTER", "QUADRATIC", "AS STORED"):
        assert said in section, said                                             # the semantics the header has to state
    make = open(os.path.join(ROOT, "vrod_amd", "csrc", "Makefile")).read()
    assert "near_plan.h" in make and "kernels_near.hip" in make


def test_stats_struct_is_eight_words(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_near_stats) == 64, "vrod_near_stats");\n'
                   + "".join('_Static_assert(offsetof(vrod_near_stats, %s) == %d, "%s");\n' % (f, 8 * i, f) for i, f in enumerate(FIELDS))
                   + '_Static_assert(VROD_NEAR_SMALL_POOL == 0x80000000u, "flag");\n'
                   'int (*find)(vrod_index *, float, uint32_t, uint64_t *, uint64_t, vrod_near_stats *) = vrod_index_find_near_duplicates;\n'
                   'int (*find_d)(vrod_index *, float, uint32_t, uint64_t *, uint64_t, vrod_near_stats *, void *) = vrod_index_find_near_duplicates_device;\n'
                   'int (*del)(vrod_index *, float, uint32_t, uint64_t *) = vrod_index_delete_near_duplicates;\n'
                   'int main(void) { vrod_near_stats s = {0}; return (int)s.rows; }\n')
    lib = os.path.join(ROOT, "vrod_amd", "libvrod_hip.so")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")], check=True)
    assert os.path.exists(lib)


def test_argument_validation_without_device():
    """A null handle is refused by every entry point whatever else it is given, and no output is written."""
    import vrod_amd
    from vrod_amd._lib import NearStats
    L = vrod_amd.load()
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    st = NearStats(*([9] * 8))
    n = C.c_uint64(7)
    for thr in (0.5, float("nan"), float("inf")):
        for flags in (0, 1, 0x80000000, 0x80000001, 0xFFFFFFFF):
            for map_len in (0, 4):
                assert L.vrod_index_find_near_duplicates(None, thr, flags, out, map_len, C.byref(st)) == 1
                assert L.vrod_index_find_near_duplicates(None, thr, flags, None, map_len, None) == 1
                assert L.vrod_index_find_near_duplicates_device(None, thr, flags, out, map_len, C.byref(st), None) == 1
            assert L.vrod_index_delete_near_duplicates(None, thr, flags, C.byref(n)) == 1
            assert L.vrod_index_delete_near_duplicates(None, thr, flags, None) == 1
    assert list(out) == [7, 7, 7, 7] and n.value == 7 and all(getattr(st, f) == 9 for f in FIELDS)
    assert L.vrod_last_error()


def test_wrappers_check_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, None, 0
    for call in (lambda: ix.find_near_duplicates("0.9"), lambda: ix.find_near_duplicates(None), lambda: ix.find_near_duplicates(True),
                 lambda: ix.find_near_duplicates(0.9, small_pool=1), lambda: ix.find_near_duplicates_device(0.9, small_pool="yes"),
                 lambda: ix.delete_near_duplicates([0.9])):
        with pytest.raises(TypeError):
            call()
    assert vrod_amd.Index._near_args(0.5, True) == (0.5, 0x80000000) and vrod_amd.Index._near_args(np.float32(0.25)) == (0.25, 0)
    assert vrod_amd.Index._near_args(1)[0] == 1.0 and np.isnan(vrod_amd.Index._near_args(float("nan"))[0])   # NaN is the library's to refuse
    assert vrod_amd.Index._near_args(0.1)[0] == float(np.float32(0.1))           # the fp32 value the library will compare with
