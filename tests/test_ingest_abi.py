"""CPU tests of the device-resident ingest (vrod_index_add_device, _update_device, _upsert_device, _get_rows_device): the
symbols are exported and bound, the refusals that need no device, and the Python wrapper's own checks."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

NAMES = ["vrod_index_add_device", "vrod_index_update_device", "vrod_index_upsert_device", "vrod_index_get_rows_device"]
INVALID_ARG, NO_DEVICE = 1, 3


def test_symbols_are_exported_and_bound():
    import vrod_amd
    L = vrod_amd.load()
    out = subprocess.run(["nm", "-D", "--defined-only", vrod_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vrod_[a-z_0-9]+)", out))
    for name in NAMES:
        assert name in exported and name in vrod_amd.SYMBOLS, name
        assert getattr(L, name).restype is C.c_int
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [6, 7, 8, 6]


def test_ingest_argument_validation_without_device():
    """Null handle, null rows, an unknown element type and a bad stride are refused before any device call, so the
    answers are the same on a machine without a GPU; nothing the pointers name is touched."""
    import vrod_amd
    L = vrod_amd.load()
    rows = (C.c_float * 8)(*([7.0] * 8))     # host memory standing in for device memory: never dereferenced here
    ids = (C.c_uint64 * 2)(0, 1)
    out = (C.c_uint64 * 2)(5, 5)

    def why():
        return L.vrod_last_error().decode()

    for dt in (0, 1, 2):
        for stride in (0, 4, 1 << 63):
            assert L.vrod_index_add_device(None, rows, dt, stride, 2, None) == INVALID_ARG and "idx is null" in why()
            assert L.vrod_index_update_device(None, ids, rows, dt, stride, 2, None) == INVALID_ARG and "idx is null" in why()
            assert L.vrod_index_upsert_device(None, ids, rows, dt, stride, 2, out, None) == INVALID_ARG and "idx is null" in why()
    assert L.vrod_index_get_rows_device(None, 0, 2, rows, 4, None) == INVALID_ARG and "idx is null" in why()
    for dt in (3, -1, 255):                  # the element type is checked first: the message names it
        assert L.vrod_index_add_device(None, rows, dt, 4, 2, None) == INVALID_ARG and "src_dtype" in why()
        assert L.vrod_index_update_device(None, ids, rows, dt, 4, 2, None) == INVALID_ARG and "src_dtype" in why()
        assert L.vrod_index_upsert_device(None, ids, rows, dt, 4, 2, out, None) == INVALID_ARG and "src_dtype" in why()
    assert list(rows) == [7.0] * 8 and list(out) == [5, 5]


def test_no_device_is_the_host_forms_error():
    """Without a device no handle exists: create answers VROD_ERR_NO_DEVICE, and the device forms answer a null handle
    exactly as vrod_index_add / _update / _upsert / _get_rows do."""
    import torch
    import vrod_amd
    L = vrod_amd.load()
    rows = (C.c_float * 4)(1, 2, 3, 4)
    ids = (C.c_uint64 * 1)(0)
    if not torch.cuda.is_available():
        h = C.c_void_p()
        dev = (C.c_int * 1)(0)
        assert L.vrod_index_create(C.byref(h), 4, 0, 0, dev, 1) == NO_DEVICE and not h
    host = [L.vrod_index_add(None, rows, 1), L.vrod_index_update(None, ids, rows, 1), L.vrod_index_upsert(None, ids, rows, 1, None),
            L.vrod_index_get_rows(None, 0, 1, rows)]
    device = [L.vrod_index_add_device(None, rows, 0, 4, 1, None), L.vrod_index_update_device(None, ids, rows, 0, 4, 1, None),
              L.vrod_index_upsert_device(None, ids, rows, 0, 4, 1, None, None), L.vrod_index_get_rows_device(None, 0, 1, rows, 4, None)]
    assert host == device == [INVALID_ARG] * 4


def test_wrapper_rejects_what_it_cannot_pass_through():
    import torch
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L, ix.device = 4, None, None, 0
    ids = torch.zeros(2, dtype=torch.int64)
    calls = [lambda t: ix.add_device(t), lambda t: ix.update_device(ids, t), lambda t: ix.upsert_device(ids, t),
             lambda t: ix.get_rows_device(0, 2, out=t)]
    for call in calls:
        with pytest.raises(ValueError, match="on the GPU"):
            call(torch.zeros(2, 4))                                   # a CPU tensor
        with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
            call(torch.zeros(2, 8)[:, ::2])                           # a non-unit inner stride
        with pytest.raises(ValueError, match=r"stride\(1\) == 1"):
            call(torch.zeros(4, 2).t())
        for dt in (torch.int32, torch.int64, torch.uint8, torch.float64):
            with pytest.raises(ValueError, match="float32, bfloat16 or float16"):
                call(torch.zeros(2, 4, dtype=dt))
        with pytest.raises(ValueError, match=r"\[n, 4\]"):
            call(torch.zeros(2, 5))
        with pytest.raises(ValueError, match=r"\[n, 4\]"):
            call(torch.zeros(8))
        with pytest.raises(ValueError, match="torch tensor"):
            call(np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match=r"stride\(0\) >= 4"):
        ix.add_device(torch.zeros(1, 4).expand(3, 4))                 # stride(0) == 0
    assert (vrod_amd.SRC_F32, vrod_amd.SRC_BF16, vrod_amd.SRC_F16) == (0, 1, 2)
