"""CPU tests of the diversified search's entry points (vrod_search_diverse, vrod_search_diverse_device): declared,
exported, prototyped, present in the Rust crate, wrapped in Python -- and every VROD_ERR_INVALID_ARG the arguments alone
decide is returned without a device (without a handle, even), with the outputs untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vrod_search_diverse", "vrod_search_diverse_device")


def test_symbols_are_declared_exported_and_prototyped():
    import vrod_amd
    raw = open(os.path.join(ROOT, "include", "vrod.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = vrod_amd.load()
    out = subprocess.run(["nm", "-D", "--defined-only", vrod_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert name in vrod_amd.SYMBOLS
        assert re.search(rf" T {name}$", out, flags=re.M), name
        assert getattr(L, name).restype is C.c_int
    assert re.search(r"#define VROD_MAX_DIVERSE_POOL 1024u", hdr)
    vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
    assert L.vrod_search_diverse.argtypes == [vp, vp, u32, u32, u32, f32, vp, vp, vp]
    assert L.vrod_search_diverse_device.argtypes == [vp, vp, u32, u32, u32, f32, vp, vp, vp, vp]
    # the header's parameter lists, in order
    for name, tail in ((NAMES[0], ["out_ids", "out_scores", "out_mmr"]), (NAMES[1], ["d_out_ids", "d_out_scores", "d_out_mmr", "stream"])):
        args = re.search(rf"\bint {name}\s*\(([^;]*)\);", hdr).group(1)
        names = [a.strip().split()[-1].lstrip("*") for a in args.split(",")]
        assert names[2:6] == ["nq", "k", "pool", "lambda"] and names[6:] == tail, names


def test_rust_crate_declares_them():
    src = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    ext = src[src.index('extern "C" {'):]
    ext = ext[:ext.index("\n}\n")]
    for name in NAMES:
        assert re.search(rf"pub fn {name}\s*\(([^;]*)\) -> c_int;", ext), name
    args = re.search(r"pub fn vrod_search_diverse_device\s*\(([^;]*)\)", ext).group(1)
    assert "pool: u32" in args and "lambda: f32" in args and "d_out_mmr: *mut f32" in args and "stream: *mut c_void" in args
    args = re.search(r"pub fn vrod_search_diverse\s*\(([^;]*)\)", ext).group(1)
    assert "pool: u32" in args and "lambda: f32" in args and "out_mmr: *mut f32" in args
    assert "pub const VROD_MAX_DIVERSE_POOL: u32 = 1024;" in src


def test_every_invalid_arg_returns_without_a_device_and_writes_nothing():
    import vrod_amd
    L = vrod_amd.load()
    q = (C.c_float * 8)()
    n = 4 * 1100
    ids = np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64)
    sc = np.full(n, -12345.5, np.float32)
    mmr = np.full(n, -777.25, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nan = float("nan")
    cases = [
        (0, 10, 0.5, "k must be"), (11, 10, 0.5, "larger than the pool"), (1100, 1024, 0.5, "larger than the pool"),
        (10, 1025, 0.5, "pool must be"), (1025, 1025, 0.5, "pool must be"),
        (10, 10, nan, "lambda"), (10, 10, -0.001, "lambda"), (10, 10, 1.001, "lambda"), (10, 10, float("inf"), "lambda"),
    ]
    for k, pool, lam, text in cases:   # (the message tells which check refused: the arguments', not the null handle's)
        assert L.vrod_search_diverse(None, q, 2, k, pool, lam, p(ids), p(sc), p(mmr)) == 1, (k, pool, lam)
        assert text in L.vrod_last_error().decode(), (k, pool, lam, L.vrod_last_error())
        assert L.vrod_search_diverse_device(None, q, 2, k, pool, lam, p(ids), p(sc), p(mmr), None) == 1, (k, pool, lam)
        assert text in L.vrod_last_error().decode()
        assert L.vrod_search_diverse(None, q, 0, k, pool, lam, None, None, None) == 1     # ... and before nq == 0 is OK
        assert text in L.vrod_last_error().decode()
    # a null handle, with arguments that are fine
    assert L.vrod_search_diverse(None, q, 2, 2, 4, 0.5, p(ids), p(sc), p(mmr)) == 1
    assert "idx is null" in L.vrod_last_error().decode()
    assert L.vrod_search_diverse_device(None, q, 2, 2, 4, 0.5, p(ids), p(sc), None, None) == 1
    assert L.vrod_search_diverse(None, None, 0, 2, 4, 0.5, None, None, None) == 1
    assert (ids == 0x5A5A5A5A5A5A5A5A).all() and (sc == np.float32(-12345.5)).all() and (mmr == np.float32(-777.25)).all()


def test_python_wrappers_exist_and_check_their_shapes():
    import vrod_amd
    from vrod_amd import index as I
    assert callable(vrod_amd.Index.search_diverse) and callable(vrod_amd.Index.search_diverse_device)
    assert I.MAX_DIVERSE_POOL == 1024
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, vrod_amd.load()
    with pytest.raises(ValueError):
        ix.search_diverse(np.zeros((3, 5), np.float32), 2, 4, 0.5)           # queries of the wrong width
    with pytest.raises(ValueError):
        ix.search_diverse(np.zeros((2, 3, 4), np.float32), 2, 4, 0.5)        # not a matrix
    with pytest.raises(vrod_amd.VrodError) as e:                             # the library's own refusal comes through
        ix.search_diverse(np.zeros((3, 4), np.float32), 5, 4, 0.5)
    assert e.value.code == 1 and "pool" in str(e.value)
    with pytest.raises(vrod_amd.VrodError) as e:
        ix.search_diverse(np.zeros(4, np.float32), 2, 4, 1.5)                # a single query as a vector; lambda refused
    assert e.value.code == 1 and "lambda" in str(e.value)
