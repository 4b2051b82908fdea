"""CPU tests of the search by weighted examples (vrod_search_combined, vrod_search_combined_device): the refusals that the
arguments alone decide, which need no device, with the outputs left as they were; and the Python wrapper's own checks."""
import ctypes as C

import numpy as np
import pytest

SENT_ID, SENT_SC = 0x5A5A5A5A5A5A5A5A, -12345.5


def test_combined_argument_validation_without_device():
    import vrod_amd
    L = vrod_amd.load()
    tl = (C.c_uint32 * 2)(0, 1)
    tid = (C.c_uint64 * 1)(0)
    tw = (C.c_float * 1)(1.0)
    oi = (C.c_uint64 * 16)(*([SENT_ID] * 16))
    sc = (C.c_float * 16)(*([SENT_SC] * 16))
    ex = vrod_amd.index.COMBINED_EXCLUDE_TERMS

    def why():
        return L.vrod_last_error().decode()

    def host(k, flags, tl=tl, oi=oi, sc=sc):
        return L.vrod_search_combined(None, None, None, tl, tid, tw, None, None, 1, k, flags, oi, sc)

    def device(k, flags, tl=tl, oi=oi, sc=sc):
        return L.vrod_search_combined_device(None, None, None, tl, tid, tw, None, None, 1, k, flags, oi, sc, None)

    for call in (host, device):
        # a null handle, null buffers
        assert call(1, 0) == 1
        assert call(1, 0, tl=None, oi=None, sc=None) == 1
        # what the arguments alone decide is checked before the handle, so it can be told apart here by its message
        for flags in (2, 0x80000001, 0xFFFFFFFE):
            assert call(1, flags) == 1 and "unknown flag bits" in why()
        for k in (0, vrod_amd.MAX_K + 1):
            for flags in (0, ex):
                assert call(k, flags) == 1 and "k must be in" in why()
        # ... and arguments that pass those checks get as far as the handle
        assert call(vrod_amd.MAX_K, 0) == 1 and "idx is null" in why()
        assert call(1, ex) == 1 and "idx is null" in why()
    assert all(x == SENT_ID for x in oi) and all(x == SENT_SC for x in sc)
    assert L.vrod_last_error()


def test_wrapper_rejects_malformed_arguments_before_the_library():
    import vrod_amd
    ix = vrod_amd.Index.__new__(vrod_amd.Index)   # no device here: only the wrapper's own checks run
    ix.dim, ix._h, ix._L = 4, None, None
    with pytest.raises(TypeError):
        ix.search_combined(2, [[0.5]], [[1.0]])
    with pytest.raises(ValueError):
        ix.search_combined(2, [[-1]], [[1.0]])
    with pytest.raises(ValueError):
        ix.search_combined(2, [[1, 2]], [[1.0]])                                     # a weight per term
    with pytest.raises(ValueError):
        ix.search_combined(2, [1, 2], [1.0, 1.0], term_lims=[0, 1])                   # lims[-1] is the number of ids
    with pytest.raises(ValueError):
        ix.search_combined(2, [[1]], [[1.0]], vectors=np.zeros((2, 4), np.float32))   # a vector per query
    with pytest.raises(ValueError):
        ix.search_combined(2, [[1]], [[1.0]], vectors=np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        ix.search_combined(2, [[1]], [[1.0]], vectors=np.zeros((1, 4), np.float32), vector_weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        ix.search_combined(2, [[1]], [[1.0]], exclude_ids=[[1], [2]])                 # an exclude list per query
    ids, lims = vrod_amd.Index._ragged_ids([[1, 2], [], [1 << 40]], None, "term")
    assert ids.dtype == np.uint64 and ids.tolist() == [1, 2, 1 << 40] and lims.dtype == np.uint32 and lims.tolist() == [0, 2, 2, 3]
    ids, lims = vrod_amd.Index._ragged_ids([], None, "term")
    assert ids.size == 0 and lims.tolist() == [0]
