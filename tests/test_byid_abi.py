"""CPU tests of the searches by stored row (vrod_search_by_ids, vrod_search_by_ids_device, vrod_knn_graph): argument
validation that needs no device, and the Python wrappers' own checks."""
import ctypes as C

import numpy as np
import pytest


def test_byid_argument_validation_without_device():
    import vrod_amd
    L = vrod_amd.load()
    ids = (C.c_uint64 * 4)()
    oi = (C.c_uint64 * 16)()
    sc = (C.c_float * 16)()
    # a null handle, null buffers
    assert L.vrod_search_by_ids(None, ids, 1, 1, 0, oi, sc) == 1
    assert L.vrod_search_by_ids(None, None, 1, 1, 0, None, None) == 1
    assert L.vrod_search_by_ids_device(None, ids, 1, 1, 0, oi, sc, None) == 1
    assert L.vrod_search_by_ids_device(None, None, 1, 1, 0, None, None, None) == 1
    assert L.vrod_knn_graph(None, 0, 1, 1, oi, sc) == 1
    assert L.vrod_knn_graph(None, 0, 1, 1, None, None) == 1
    # What the arguments alone decide is checked before the handle, so that it can be told apart here by its message:
    # unknown flag bits, k = VROD_MAX_K with the self drop, k = 0, k past VROD_MAX_K.
    ex = vrod_amd.index.BYID_EXCLUDE_SELF

    def why():
        return L.vrod_last_error().decode()

    for flags in (2, 0x80000001, 0xFFFFFFFE):
        assert L.vrod_search_by_ids(None, ids, 1, 1, flags, oi, sc) == 1 and "unknown flag bits" in why()
        assert L.vrod_search_by_ids_device(None, ids, 1, 1, flags, oi, sc, None) == 1 and "unknown flag bits" in why()
    assert L.vrod_search_by_ids(None, ids, 1, vrod_amd.MAX_K, ex, oi, sc) == 1 and "k must be in" in why()
    assert L.vrod_search_by_ids_device(None, ids, 1, vrod_amd.MAX_K, ex, oi, sc, None) == 1 and "k must be in" in why()
    assert L.vrod_knn_graph(None, 0, 1, vrod_amd.MAX_K, oi, sc) == 1 and "k must be in" in why()
    assert L.vrod_search_by_ids(None, ids, 1, vrod_amd.MAX_K + 1, 0, oi, sc) == 1 and "k must be in" in why()
    assert L.vrod_knn_graph(None, 0, 1, 0, oi, sc) == 1 and "k must be in" in why()
    assert L.vrod_search_by_ids(None, ids, 1, 0, 0, oi, sc) == 1 and "k must be in" in why()
    # ... and arguments that pass those checks get as far as the handle
    assert L.vrod_search_by_ids(None, ids, 1, vrod_amd.MAX_K, 0, oi, sc) == 1 and "idx is null" in why()
    assert L.vrod_search_by_ids(None, ids, 1, vrod_amd.MAX_K - 1, ex, oi, sc) == 1 and "idx is null" in why()
    assert L.vrod_knn_graph(None, 0, 1, vrod_amd.MAX_K - 1, oi, sc) == 1 and "idx is null" in why()
    assert L.vrod_last_error()


def test_wrappers_reject_bad_ids_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    with pytest.raises(TypeError):
        ix.search_by_ids(np.zeros(3, np.float32), 2)
    with pytest.raises(TypeError):
        ix.search_by_ids([0.5, 1.0], 2)
    with pytest.raises(TypeError):
        ix.search_by_ids(np.zeros(3, bool), 2)
    with pytest.raises(ValueError):
        ix.search_by_ids(np.array([3, -1]), 2)
    with pytest.raises(ValueError):
        ix.search_by_ids([-5], 2, exclude_self=True)
    with pytest.raises(ValueError):
        ix.knn_graph(2, first_id=-1, n=1)
    with pytest.raises(ValueError):
        ix.knn_graph(2, first_id=0, n=-1)
    with pytest.raises(ValueError):
        ix.knn_graph(2, n=5)
    a = vrod_amd.Index._query_ids(np.array([[1, 2], [3, 1 << 40]], np.int64))
    assert a.dtype == np.uint64 and a.tolist() == [1, 2, 3, 1 << 40] and a.flags.c_contiguous
    assert vrod_amd.Index._query_ids([1, 1 << 63]).tolist() == [1, 1 << 63]
    assert vrod_amd.Index._query_ids([]).size == 0
