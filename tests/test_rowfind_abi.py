"""CPU tests of the row-lookup entry points (vrod_index_find_rows, _find_rows_device, _add_unique, _add_unique_device): the
four names in every layer, the stats struct's layout, argument validation that needs no device, and the Python wrappers'
own checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rowfind_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
NAMES = ["vrod_index_find_rows", "vrod_index_find_rows_device", "vrod_index_add_unique", "vrod_index_add_unique_device"]
FIELDS = ["rows", "found", "repeats", "appended", "batches", "slots", "max_probe", "compare_misses"]
ERR_INVALID_ARG = 1


def test_names_in_every_layer():
    import vrod_amd
    from vrod_amd._lib import RowfindStats
    L = vrod_amd.load()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ps = C.POINTER(RowfindStats)
    host, device = [vp, vp, u64, u32, vp, ps], [vp, vp, i32, u64, u64, u32, vp, ps, vp]
    for name, argtypes in zip(NAMES, (host, device, host, device)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in vrod.h"
        assert name in vrod_amd.SYMBOLS and hasattr(L, name), name
        assert list(getattr(L, name).argtypes) == argtypes, name
        assert getattr(L, name).restype in (C.c_int, C.c_int32), name
        assert re.search(r"\bpub fn %s\s*\(" % name, rust), f"{name} is not in the Rust binding"
    assert [f for f, _ in RowfindStats._fields_] == FIELDS and C.sizeof(RowfindStats) == 64
    assert re.search(r"typedef struct\s*\{\s*" + r"[^}]*".join(r"uint64_t\s+%s[;,]" % f for f in FIELDS) + r"[^}]*\}\s*vrod_rowfind_stats;", header)
    assert re.search(r"pub struct vrod_rowfind_stats\s*\{\s*" + r"\s*".join(r"pub %s: u64," % f for f in FIELDS) + r"\s*\}", rust)
    assert re.search(r"#define VROD_ROWFIND_NARROW_HASH 0x80000000u", header) and re.search(r"#define VROD_ROWFIND_SMALL_BATCH 0x40000000u", header)
    assert re.search(r"pub const VROD_ROWFIND_NARROW_HASH: u32 = 0x8000_0000;", rust) and re.search(r"pub const VROD_ROWFIND_SMALL_BATCH: u32 = 0x4000_0000;", rust)
    assert (vrod_amd.ROWFIND_NARROW_HASH, vrod_amd.ROWFIND_SMALL_BATCH) == (rowfind_model.ROWFIND_NARROW_HASH, rowfind_model.ROWFIND_SMALL_BATCH)
    assert (vrod_amd.ROWFIND_NARROW_HASH, vrod_amd.ROWFIND_SMALL_BATCH) == (0x80000000, 0x40000000)
    for method in ("find_rows", "find_rows_device", "add_unique", "add_unique_device"):
        assert callable(getattr(vrod_amd.Index, method))
    section = header[header.index("/* Row lookup"):header.index("#define VROD_ROWFIND_NARROW_HASH")]
    for said in ("SMALLEST ID", "DIAGNOSTICS", "-0.0", "VROD_ERR_INVALID_VALUE", "VROD_ERR_UNSUPPORTED", "VROD_ERR_INTERNAL", "16 bytes"):
        assert said in section, said
    makefile = open(os.path.join(ROOT, "vrod_amd", "csrc", "Makefile")).read()
    assert "kernels_rowfind.hip" in makefile and "rowfind_plan.h" in makefile


def test_stats_struct_is_eight_words(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "vrod.h"\n_Static_assert(sizeof(vrod_rowfind_stats) == 64, "vrod_rowfind_stats");\n'
                   + "".join('_Static_assert(offsetof(vrod_rowfind_stats, %s) == %d, "%s");\n' % (f, 8 * i, f) for i, f in enumerate(FIELDS))
                   + '_Static_assert(VROD_ROWFIND_NARROW_HASH == 0x80000000u && VROD_ROWFIND_SMALL_BATCH == 0x40000000u, "flags");\n'
                   'int main(void) { vrod_rowfind_stats s = {0}; return (int)s.rows; }\n')
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")], check=True)
    subprocess.run([str(tmp_path / "size")], check=True)


def test_argument_validation_without_device():
    """A null handle, null rows with n > 0 and unknown flag bits are refused by every entry point, and no output is written."""
    import vrod_amd
    from vrod_amd._lib import RowfindStats
    L = vrod_amd.load()
    rows = np.ones((4, 8), np.float32)
    p = rows.ctypes.data_as(vp)
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    st = RowfindStats(*([9] * 8))
    for host, device in ((L.vrod_index_find_rows, L.vrod_index_find_rows_device), (L.vrod_index_add_unique, L.vrod_index_add_unique_device)):
        for flags in (0, 1, 2, 0x20000000, 0x40000000, 0x80000000, 0xC0000000, 0xC0000001, 0xFFFFFFFF):
            for n in (0, 4):
                assert host(None, p, n, flags, out, C.byref(st)) == ERR_INVALID_ARG                 # a null handle
                assert host(None, None, n, flags, None, None) == ERR_INVALID_ARG
                for src_dtype in (0, 1, 2, 7):
                    assert device(None, p, src_dtype, 8, n, flags, out, C.byref(st), None) == ERR_INVALID_ARG
                assert device(None, None, 0, 8, n, flags, None, None, None) == ERR_INVALID_ARG
            assert host(None, None, 4, flags, out, C.byref(st)) == ERR_INVALID_ARG                  # null rows with n > 0
            assert device(None, None, 0, 8, 4, flags, out, C.byref(st), None) == ERR_INVALID_ARG
            assert device(None, p, 0, 7, 4, flags, out, C.byref(st), None) == ERR_INVALID_ARG       # a stride below dim would come next
    assert list(out) == [7, 7, 7, 7] and all(getattr(st, f) == 9 for f in FIELDS)
    assert L.vrod_last_error()


def test_wrappers_check_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, vrod_amd.load(), 0
    rows = np.ones((3, 4), np.float32)
    for call in (lambda: ix.find_rows(rows, narrow_hash=1), lambda: ix.find_rows(rows, small_batch="yes"), lambda: ix.add_unique(rows, narrow_hash=None),
                 lambda: ix.add_unique(rows, small_batch=0), lambda: ix.find_rows_device(None, narrow_hash=2), lambda: ix.add_unique_device(None, small_batch=1)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: ix.find_rows(np.ones((3, 5), np.float32)), lambda: ix.add_unique(np.ones(4, np.float32)), lambda: ix.find_rows_device(rows),
                 lambda: ix.add_unique_device(rows)):
        with pytest.raises(ValueError):
            call()
    assert vrod_amd.Index._rowfind_flags(True, True) == 0xC0000000 and vrod_amd.Index._rowfind_flags() == 0
    assert vrod_amd.Index._rowfind_flags(np.bool_(True)) == 0x80000000 and vrod_amd.Index._rowfind_flags(small_batch=True) == 0x40000000
    with pytest.raises(vrod_amd.VrodError) as e:   # the library refuses a null handle: the wrapper passes the code on
        ix.find_rows(rows)
    assert e.value.code == ERR_INVALID_ARG
