"""CPU tests of the candidate-list searches (vrod_search_candidates, vrod_score_candidates and their _device forms): the
symbols are exported, the refusals that need no device leave the outputs as they were, and the Python wrapper checks what it
can before it calls the library."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

SENT_ID, SENT_SC = 0x5A5A5A5A5A5A5A5A, -12345.5
NAMES = ["vrod_search_candidates", "vrod_search_candidates_device", "vrod_score_candidates", "vrod_score_candidates_device"]


def test_symbols_are_exported_and_bound():
    import vrod_amd
    L = vrod_amd.load()
    out = subprocess.run(["nm", "-D", "--defined-only", vrod_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (vrod_[a-z_0-9]+)", out))
    for name in NAMES:
        assert name in exported and name in vrod_amd.SYMBOLS, name
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes, name
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [8, 9, 6, 7]


def test_candidates_argument_validation_without_device():
    import vrod_amd
    L = vrod_amd.load()
    q = (C.c_float * 4)(1, 0, 0, 0)
    lims = (C.c_uint32 * 2)(0, 1)
    cid = (C.c_uint64 * 1)(0)
    oi = (C.c_uint64 * 16)(*([SENT_ID] * 16))
    sc = (C.c_float * 16)(*([SENT_SC] * 16))

    def why():
        return L.vrod_last_error().decode()

    calls = [
        lambda k: L.vrod_search_candidates(None, q, 1, k, lims, cid, oi, sc),
        lambda k: L.vrod_search_candidates_device(None, q, 1, k, lims, cid, oi, sc, None),
        lambda k: L.vrod_score_candidates(None, q, 1, lims, cid, sc),
        lambda k: L.vrod_score_candidates_device(None, q, 1, lims, cid, sc, None),
    ]
    for call in calls:
        for k in (1, 0, vrod_amd.MAX_K, vrod_amd.MAX_K + 1):
            assert call(k) == 1 and "idx is null" in why()     # a null handle is refused whatever else is passed
    assert all(x == SENT_ID for x in oi) and all(x == SENT_SC for x in sc)


def test_wrapper_rejects_malformed_arguments_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    q = np.zeros((2, 4), np.float32)
    for call in (lambda *a, **kw: ix.search_candidates(q, 3, *a, **kw), lambda *a, **kw: ix.score_candidates(q, *a, **kw)):
        with pytest.raises(ValueError):
            call([[1], [2], [3]])                              # a list per query
        with pytest.raises(ValueError):
            call([[1]])
        with pytest.raises(TypeError):
            call([[0.5], [1]])
        with pytest.raises(ValueError):
            call([[-1], [1]])
        with pytest.raises(ValueError):
            call([1, 2, 3], cand_lims=[0, 1, 2])               # lims[-1] is the number of ids
        with pytest.raises(ValueError):
            call([1, 2, 3], cand_lims=[0, 3])                  # nq + 1 entries
    with pytest.raises(ValueError):
        ix.search_candidates(np.zeros((2, 3), np.float32), 3, [[1], [2]])
    assert vrod_amd.index.MAX_CANDIDATES == 16384
