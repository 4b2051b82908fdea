"""CPU tests of the row-label entry points (vrod_index_set_labels, vrod_index_get_labels, vrod_search_labeled,
vrod_search_labeled_device): argument validation that needs no device, and the Python wrappers' own checks."""
import ctypes as C

import numpy as np
import pytest


def test_label_argument_validation_without_device():
    import vrod_amd
    L = vrod_amd.load()
    buf = (C.c_uint32 * 4)()
    q = (C.c_float * 4)()
    ids = (C.c_uint64 * 4)()
    sc = (C.c_float * 4)()
    assert L.vrod_index_set_labels(None, 0, buf, 4) == 1
    assert L.vrod_index_set_labels(None, 0, None, 0) == 1
    assert L.vrod_index_get_labels(None, 0, 4, buf) == 1
    assert L.vrod_index_get_labels(None, 0, 0, None) == 1
    assert L.vrod_search_labeled(None, q, 1, 1, buf, ids, sc) == 1
    assert L.vrod_search_labeled(None, None, 1, 1, None, None, None) == 1
    assert L.vrod_search_labeled_device(None, q, 1, 1, buf, ids, sc, None) == 1
    assert L.vrod_search_labeled_device(None, None, 1, 1, None, None, None, None) == 1
    assert L.vrod_last_error()


def test_wrappers_reject_bad_label_arrays():
    import vrod_amd
    f = vrod_amd.Index._labels
    with pytest.raises(TypeError):
        f(np.zeros(4, np.float32))
    with pytest.raises(TypeError):
        f(np.zeros(4, bool))
    with pytest.raises(TypeError):
        f([0.5, 1.0])
    with pytest.raises(ValueError):
        f(np.zeros(3, np.uint32), 4)
    with pytest.raises(ValueError):
        f(np.array([-1, 2]))
    with pytest.raises(ValueError):
        f(np.array([1 << 32], np.uint64))
    a = f(np.array([[1, 2], [3, 0xFFFFFFFF]], np.int64), 4)
    assert a.dtype == np.uint32 and a.tolist() == [1, 2, 3, 0xFFFFFFFF] and a.flags.c_contiguous
    assert f([], 0).size == 0 and f([], 0).dtype == np.uint32


def test_search_labeled_checks_labels_before_the_library():
    """search_labeled validates the label vector against the batch before it calls into the library."""
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    q = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError):
        ix.search_labeled(q, 2, np.zeros(2, np.uint32))
    with pytest.raises(TypeError):
        ix.search_labeled(q, 2, np.zeros(3, np.float64))
