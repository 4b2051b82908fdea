"""rowpred_model.RowPredModelIndex against brute-force Python: one row at a time, Python ints only, on the edge values the
GPU tests use (INT64_MIN / INT64_MAX, bit 63 of the tags, label 0xFFFFFFFF), under deletions, a filter and an id offset."""
import numpy as np
import pytest

from index_model import ModelError
from rowpred_model import ALLOWED, MATCH_ALL, RowPredModelIndex
from where_model import I64_MAX, I64_MIN

B63 = 1 << 63
N, DIM, OFF = 90, 4, 700
VALUES = [-7, -3, -1, 0, 2, 5, I64_MIN, I64_MAX]
LABELS = [0, 1, 7, 0xFFFFFFFF]
PREDS = [
    MATCH_ALL,
    (1, 0, 0, I64_MIN, I64_MAX, 0, 0), (0, 3, 0, I64_MIN, I64_MAX, 0, 0), (0, 0, 4, I64_MIN, I64_MAX, 0, 0), (B63, 0, 0, I64_MIN, I64_MAX, 0, 0),
    (0, 0, 0, -3, 2, 0, 0), (0, 0, 0, I64_MIN, I64_MIN, 0, 0), (0, 0, 0, I64_MAX, I64_MAX, 0, 0), (0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, I64_MIN, I64_MAX, 7, 1), (0, 0, 0, I64_MIN, I64_MAX, 0xFFFFFFFF, 1), (0, 0, 0, I64_MIN, I64_MAX, 0, 1),
    (0, 0, 0, I64_MIN, I64_MAX, 7, 0),                                           # a label that is not compared
    (6, 1, B63, -7, 5, 1, 1), (B63 | 1, 0, 2, -1, I64_MAX, 0xFFFFFFFF, 1),
    (0, 1, 1, I64_MIN, I64_MAX, 0, 0), (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, I64_MAX, I64_MIN, 7, 1),   # unsatisfiable
    (0, 0, 0, 6, I64_MAX - 1, 0, 0), (0, 0, 0, I64_MIN, I64_MAX, 3, 1),          # satisfiable, no row
]


def brute(model, pred, scope):
    """Local rows, ascending: `scope` is 'live', 'allowed' (live and allowed) or 'all'."""
    a, b, c, lo, hi, label, has = pred
    out = []
    for r in range(model.count):
        t, v, l = int(model.tags[r]), int(model.values[r]), int(model.labels[r])
        ok = (a == 0 or (t & a) != 0) and (t & b) == b and (t & c) == 0 and lo <= v <= hi and (not has or l == label)
        if scope != "all" and model.deleted[r]:
            ok = False
        if scope == "allowed" and model.allow is not None and not model.allow[r]:
            ok = False
        if ok:
            out.append(r)
    return out


@pytest.fixture()
def model():
    rng = np.random.default_rng(5)
    m = RowPredModelIndex(DIM, "f32", "l2", id_offset=OFF)
    m.add(rng.standard_normal((N, DIM)).astype(np.float32))
    m.set_tags(OFF, rng.integers(0, 8, N).astype(np.uint64) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63)))
    m.set_values(OFF, np.array(VALUES, np.int64)[rng.integers(0, len(VALUES), N)])
    m.set_labels(OFF, np.array(LABELS, np.uint32)[rng.integers(0, len(LABELS), N)])
    return m


def restrict(m):
    rng = np.random.default_rng(6)
    m.set_filter(rng.random(N - 10) < 0.7)                                       # shorter than the count: the tail is not allowed
    m.delete(rng.choice(N, 12, replace=False).astype(np.uint64) + np.uint64(OFF))


@pytest.mark.parametrize("restricted", [False, True])
def test_matching_count_and_select(model, restricted):
    if restricted:
        restrict(model)
    some = 0
    for flags, scope in ((0, "live"), (ALLOWED, "allowed")):
        want = [brute(model, p, scope) for p in PREDS]
        assert [model.matching(p, flags).tolist() for p in PREDS] == want
        assert model.count_where(PREDS, flags).tolist() == [len(w) for w in want]
        for p, w in zip(PREDS, want):
            assert model.select_where(p, flags).tolist() == [r + OFF for r in w]
        some += sum(bool(w) for w in want)
    assert some > 20
    assert model.matching(MATCH_ALL).size == model.live_count() and model.matching(MATCH_ALL, ALLOWED).size == model.filter_count()
    if restricted:
        assert model.filter_count() < model.live_count() < N
    assert model.matching((1, 0, 0, -3, 2)).tolist() == [r for r in brute(model, (1, 0, 0, -3, 2, 0, 0), "allowed")]   # the parent's form


@pytest.mark.parametrize("flags", [0, ALLOWED])
def test_delete_where(model, flags):
    restrict(model)
    for p in PREDS[9:14]:
        want = brute(model, p, "allowed" if flags else "live")
        before = model.deleted.copy()
        assert model.delete_where(p, flags) == len(want)
        assert np.flatnonzero(model.deleted & ~before).tolist() == want
        assert model.delete_where(p, flags) == 0


def test_set_filter_where(model):
    restrict(model)
    old = model.allow.copy()
    p = PREDS[5]
    model.set_filter_where(p, ALLOWED)                                           # narrows: deleted rows keep their bit
    assert np.flatnonzero(model.allow).tolist() == [r for r in brute(model, p, "all") if old[r]]
    model.set_filter_where(p, 0)                                                 # replaces
    assert np.flatnonzero(model.allow).tolist() == brute(model, p, "all")
    assert model.filter_count() == len(brute(model, p, "live"))
    model.set_filter_where(PREDS[16], 0)                                         # unsatisfiable: a filter that allows nothing
    assert model.allow is not None and not model.allow.any() and model.filter_count() == 0
    model.set_filter(None)
    model.set_filter_where(p, ALLOWED)                                           # no filter set: the flag changes nothing
    assert np.flatnonzero(model.allow).tolist() == brute(model, p, "all")


def test_set_tags_where(model):
    restrict(model)
    p = (0, 0, 0, -3, I64_MAX, 7, 1)
    rows = brute(model, p, "live")
    old = model.tags.copy()
    want = old.copy()
    changed = 0
    for r in rows:
        t = (int(old[r]) & ~(B63 | 2)) | 4
        changed += t != int(old[r])
        want[r] = t
    assert model.set_tags_where(p, 4, B63 | 2) == changed > 0
    assert np.array_equal(model.tags, want)
    assert model.set_tags_where(p, 4, B63 | 2) == 0                              # idempotent
    with pytest.raises(ModelError):
        model.set_tags_where(p, 3, 1)
    with pytest.raises(ModelError):
        model.matching((0, 0, 0, 0, 0, 0, 2), 0)
    with pytest.raises(ModelError):
        model.matching(MATCH_ALL, 2)
