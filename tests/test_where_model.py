"""where_model.WhereModelIndex pinned on hand-written cases (CPU, the oracle only): the values follow add / set / compact,
the interval is signed with both ends inclusive, INT64_MIN / INT64_MAX work as values and as bounds, lo > hi and
all & none != 0 match nothing, and search_where is the plain search over the matching rows."""
import numpy as np
import pytest

from index_model import ModelError
from support import ID_NONE, assert_same
from where_model import FULL, I64_MAX, I64_MIN, WHERE_DTYPE, WhereModelIndex, as_preds, distinct_preds, unsatisfiable, where_matches

VALUES = np.array([0, -1, 1, -5, 5, I64_MIN, I64_MAX, 7, -7, 0], np.int64)
TAGS = np.array([0, 1, 1, 2, 2, 3, 3, 1 << 63, 0, 1], np.uint64)


def rows(pred):
    return np.flatnonzero(where_matches(TAGS, VALUES, pred)).tolist()


def test_interval_is_signed_and_inclusive():
    assert rows((0, 0, 0, *FULL)) == list(range(10))
    assert rows((0, 0, 0, -5, 5)) == [0, 1, 2, 3, 4, 9]                        # both ends included, zero spanned
    assert rows((0, 0, 0, -4, 4)) == [0, 1, 2, 9]
    assert rows((0, 0, 0, 5, 5)) == [4] and rows((0, 0, 0, -5, -5)) == [3]      # a point
    assert rows((0, 0, 0, -7, -1)) == [1, 3, 8]                                # negatives only: an unsigned compare sees none
    assert rows((0, 0, 0, 1, I64_MAX)) == [2, 4, 6, 7]
    assert rows((0, 0, 0, I64_MIN, -1)) == [1, 3, 5, 8]
    assert rows((0, 0, 0, I64_MIN, I64_MIN)) == [5] and rows((0, 0, 0, I64_MAX, I64_MAX)) == [6]
    assert rows((0, 0, 0, I64_MIN + 1, I64_MAX - 1)) == [0, 1, 2, 3, 4, 7, 8, 9]


def test_tags_and_interval_are_joined():
    assert rows((1, 0, 0, *FULL)) == [1, 2, 5, 6, 9]
    assert rows((1, 0, 0, 0, I64_MAX)) == [2, 6, 9]
    assert rows((0, 3, 0, I64_MIN, 0)) == [5]
    assert rows((0, 0, 1, -7, 7)) == [0, 3, 4, 7, 8]
    assert rows((1 << 63, 0, 0, 7, 7)) == [7] and rows((1 << 63, 0, 0, 8, 9)) == []


def test_nothing_matches_an_empty_interval_or_a_contradiction():
    for p in ((0, 0, 0, 1, 0), (0, 0, 0, I64_MAX, I64_MIN), (0, 1, 1, *FULL), (1, 2, 6, -5, 5)):
        assert unsatisfiable(p) and rows(p) == []
    for p in ((0, 0, 0, 0, 0), (0, 0, 0, *FULL), (0, 1, 2, 3, 3)):
        assert not unsatisfiable(p)


def test_predicates_keep_all_64_bits_and_order_signed():
    p = as_preds([(1 << 63, 0, 0, 5, 6), (1 << 63, 0, 0, -5, 6), (1 << 63, 0, 0, I64_MIN, I64_MAX), (1 << 63, 0, 0, -5, 6)])
    assert p.dtype == WHERE_DTYPE and p.dtype.itemsize == 40 and int(p["any"][0]) == 1 << 63 and int(p["lo"][2]) == I64_MIN
    assert distinct_preds(p) == [(1 << 63, 0, 0, I64_MIN, I64_MAX), (1 << 63, 0, 0, -5, 6), (1 << 63, 0, 0, 5, 6)]


@pytest.fixture(scope="module")
def model():
    rng = np.random.default_rng(1)
    m = WhereModelIndex(8, "f32", "cosine", id_offset=100)
    m.add(rng.standard_normal((10, 8)).astype(np.float32))
    return m, rng


def test_values_follow_the_rows(model):
    m, rng = model
    assert not m.get_values(100, 10).any()                                      # 0 until set
    m.set_values(100, VALUES)
    m.set_tags(100, TAGS)
    m.add(rng.standard_normal((3, 8)).astype(np.float32))
    assert m.get_values(100, 13).tolist() == VALUES.tolist() + [0, 0, 0]         # rows added later read 0
    for first, n in ((99, 1), (112, 2), (114, 0)):
        with pytest.raises(ModelError):
            m.set_values(first, np.ones(n, np.int64))
        with pytest.raises(ModelError):
            m.get_values(first, n)
    m.set_values(113, [])                                                        # n == 0 at the end: nothing
    m.delete(np.array([101, 105], np.uint64))
    m.set_values(101, [-9])                                                      # a deleted row may be named
    assert m.get_values(101, 1).tolist() == [-9]
    rq = rng.standard_normal((4, 8)).astype(np.float32)
    preds = [(0, 0, 0, *FULL), (0, 0, 0, -7, -1), (0, 0, 0, 3, 2), (1, 0, 0, 0, I64_MAX)]
    assert m.matching(preds[1]).tolist() == [3, 8] and m.matching(preds[3]).tolist() == [2, 6, 9]    # rows 1 and 5 are deleted
    ids, sc = m.search_where(rq, 4, preds)
    assert_same(ids[:1], sc[:1], *(x[:1] for x in m.search(rq, 4)), "the full interval is the plain search")
    assert sorted(ids[1].tolist()) == [103, 108, int(ID_NONE), int(ID_NONE)] and np.isnan(sc[1, 2:]).all()
    assert (ids[2] == ID_NONE).all() and np.isnan(sc[2]).all()
    assert sorted(ids[3, :3].tolist()) == [102, 106, 109] and ids[3, 3] == ID_NONE
    m.compact()
    assert m.get_values(100, 11).tolist() == [0, 1, -5, 5, I64_MAX, 7, -7, 0, 0, 0, 0]
    assert m.get_tags(100, 11).tolist() == [0, 1, 2, 2, 3, 1 << 63, 0, 1, 0, 0, 0]
