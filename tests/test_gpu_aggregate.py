"""GPU tests of row aggregation (vrod_index_aggregate_where) against aggregate_model.AggregateModelIndex, field by field
and exactly: keys, counts, min, max, wrapping sums, first ids, the number of groups and of rows considered.

Every handle has dim 8 (the vectors matter only where a search is compared) and is reserved past its count.  The counts
sit at the wave and work-group edges of the pass (64 and 2048 rows, aggregate_plan.h); the label patterns at the corners
of the two-level table: one key for everybody (maximal contention on one LDS slot, and the folded-wave path), a few
keys, a key per row (the LDS table overflows to the global path), exactly the LDS slot count of distinct keys per
work-group and one above it, and labels chosen with the plan's hash -- restated in aggregate_model.py and pinned by
tests/test_aggregate_plan.py -- to share one home slot in BOTH tables, more of them than the LDS probe is long.
"""
import ctypes as C

import numpy as np
import pytest

from aggregate_model import (AGG_GROUP_DTYPE, BY_LABEL, BY_TAG, BY_VALUE, ERR_CAPACITY, LDS_PROBE, LDS_SLOTS, MAX_AGG_GROUPS, ORDER_COUNT, AggregateModelIndex,
                             labels_sharing_both_homes, table_slots)
from rowpred_model import ALLOWED, MATCH_ALL
from where_model import I64_MAX, I64_MIN
from support import va, assert_same  # noqa: F401

pytestmark = pytest.mark.gpu

DIM, K = 8, 10
COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 4097]
OFF = {1: 0, 63: 1000, 64: 0, 65: 1000, 2047: 0, 2048: 1000, 2049: 0, 4097: 1000}   # half of the cases carry an id offset
SENT = 0x5A5A5A5A5A5A5A5A
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 6
FULL = (I64_MIN, I64_MAX)
EXTREMES = np.array([I64_MIN, -1, 0, I64_MAX], np.int64)
ROWS_PER_GROUP = 2048                                                            # kRowPredRowsPerGroup


def colliding(n, rng):
    """More labels than the LDS probe is long, all with one home slot in the LDS table and in the global table this
    count gets: the probes walk, the last ones leave the LDS table, and every label still gets its own group."""
    return labels_sharing_both_homes(LDS_PROBE + 3, table_slots(n), like=5)[rng.permutation(n) % (LDS_PROBE + 3)]


PATTERNS = {
    "one_label": lambda n, rng: np.full(n, 0xFFFFFFFF, np.uint32),
    "mod7": lambda n, rng: (np.arange(n) % 7).astype(np.uint32),
    "own_label": lambda n, rng: rng.permutation(n).astype(np.uint32) * np.uint32(2654435761),
    "lds_slots": lambda n, rng: ((np.arange(n) % LDS_SLOTS) + (np.arange(n) // ROWS_PER_GROUP) * 100_000).astype(np.uint32),
    "lds_slots_plus_one": lambda n, rng: ((np.arange(n) % (LDS_SLOTS + 1)) + (np.arange(n) // ROWS_PER_GROUP) * 100_000).astype(np.uint32),
    "one_home": colliding,
}


def make(va, n, off=0, values=None, labels=None, tags=None, seed=0, reserve=300):
    """A handle of n rows reserved past its count, ids from `off`, and its model."""
    rng = np.random.default_rng(1000 + seed)
    rows = rng.standard_normal((n, DIM)).astype(np.float32)
    m = AggregateModelIndex(DIM, "bf16", "cosine", id_offset=off)
    ix = va.Index(DIM, "bf16", "cosine")
    ix.reserve(n + reserve)
    ix.set_id_offset(off)
    for h in (m, ix):
        if n:
            h.add(rows)
        for setter, col in ((h.set_values, values), (h.set_labels, labels), (h.set_tags, tags)):
            if col is not None and n:
                setter(off, col)
    return ix, m


def same(ix, m, pred, by, width=None, limit=None, by_count=False, allowed=False, what=""):
    """One call equals the model: every field of every group, the group count and the rows considered."""
    got, n_groups, n_rows = ix.aggregate_where(pred, by, width=width, limit=limit, by_count=by_count, allowed_only=allowed)
    want, wg, wr = m.aggregate_where(pred, by, width, limit, (ALLOWED if allowed else 0) | (ORDER_COUNT if by_count else 0))
    tag = f"{what} by{by} width{width} limit{limit} by_count{by_count} allowed{allowed}"
    assert got.dtype == AGG_GROUP_DTYPE and (n_groups, n_rows) == (wg, wr), f"{tag}: groups {n_groups} != {wg} or rows {n_rows} != {wr}"
    assert got.shape == want.shape, f"{tag}: {got.shape} != {want.shape}"
    for name in AGG_GROUP_DTYPE.names:
        assert np.array_equal(got[name], want[name]), f"{tag}: {name} differs at {np.flatnonzero(got[name] != want[name])[:5]}"
    assert n_rows == ix.count_where([pred], allowed)[0], tag                     # the rows considered are count_where's
    return got, n_groups, n_rows


def raw_call(ix, pred, flags, by, width, limit, room=8, want=(True, True, True, True)):
    """The C entry point with sentinel-filled outputs -> (rc, count, groups, rows, out)."""
    pp = pred if pred is None or isinstance(pred, np.ndarray) else ix._row_preds(pred, 1)
    out = np.full(room, SENT, np.uint64).repeat(6).view(AGG_GROUP_DTYPE)
    n, groups, rows = C.c_uint64(SENT), C.c_uint64(SENT), C.c_uint64(SENT)
    rc = ix._L.vrod_index_aggregate_where(ix._h, pp.ctypes.data if pp is not None else None, flags, by, width, limit, C.byref(n) if want[0] else None,
                                          C.byref(groups) if want[1] else None, C.byref(rows) if want[2] else None, out.ctypes.data if want[3] else None)
    return rc, n.value, groups.value, rows.value, out


def untouched(out):
    return (out.view(np.uint64) == SENT).all()


# ---------------------------------------------------------------- counts x label patterns
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_label_patterns_at_the_wave_and_group_edges(va, pattern, n):
    rng = np.random.default_rng(n * 31 + len(pattern))
    labels = PATTERNS[pattern](n, rng)
    values = rng.integers(-1000, 1000, n).astype(np.int64)
    ix, m = make(va, n, OFF[n], values, labels, seed=n)
    with ix:
        assert ix.count == n
        got, n_groups, n_rows = same(ix, m, MATCH_ALL, BY_LABEL, what=f"{pattern} n{n}")
        assert n_rows == n and int(got["count"].sum()) == n and n_groups == np.unique(labels).size
        same(ix, m, MATCH_ALL, BY_LABEL, by_count=True, what=f"{pattern} n{n}")
        same(ix, m, (0, 0, 0, -300, 500, 0, 0), BY_LABEL, limit=5, what=f"{pattern} n{n} interval")
        if pattern == "one_label":
            assert got["first_id"].tolist() == [OFF[n]] and got["key"].tolist() == [0xFFFFFFFF]
        if pattern.startswith("lds_slots") and n >= ROWS_PER_GROUP:              # exactly the slot count per work-group, and one above it
            assert np.unique(labels[:ROWS_PER_GROUP]).size == LDS_SLOTS + (pattern == "lds_slots_plus_one")
        if pattern == "one_home" and n >= 63:
            assert n_groups == LDS_PROBE + 3


def test_labels_never_set_is_one_group_with_key_zero(va):
    ix, m = make(va, 2049, 1000, values=np.arange(2049, dtype=np.int64) - 1000)
    with ix:
        got, n_groups, _ = same(ix, m, MATCH_ALL, BY_LABEL)
        assert n_groups == 1 and got.tolist() == [(0, 2049, -1000, 1048, int((np.arange(2049) - 1000).sum()), 1000)]
    ix, m = make(va, 300)                                                        # no column at all: values read 0, tags read 0
    with ix:
        assert same(ix, m, MATCH_ALL, BY_VALUE, 1)[0].tolist() == [(0, 300, 0, 0, 0, 0)]
        assert same(ix, m, MATCH_ALL, BY_TAG)[1:] == (0, 300)


# ---------------------------------------------------------------- BY_VALUE
@pytest.mark.parametrize("n", [64, 2049, 4097])
def test_by_value_extremes_and_sums_that_wrap(va, n):
    values = EXTREMES[np.arange(n) % 4]
    ix, m = make(va, n, OFF[n] if n in OFF else 0, values)
    with ix:
        got, n_groups, _ = same(ix, m, MATCH_ALL, BY_VALUE, 1, what="width 1")
        assert got["key"].tolist() == EXTREMES.tolist()                          # INT64_MIN is a key like any other
        assert int(got["count"].sum()) == n
        assert got["sum_value"][3] == np.int64((I64_MAX * int(got["count"][3]) + (1 << 63)) % (1 << 64) - (1 << 63))   # wrapped
        got, _, _ = same(ix, m, MATCH_ALL, BY_VALUE, I64_MAX, what="width INT64_MAX")
        assert got["key"].tolist() == [-2, -1, 0, 1]
        for width in (2, 86400):
            same(ix, m, MATCH_ALL, BY_VALUE, width, by_count=True)
        same(ix, m, (0, 0, 0, I64_MIN, -1, 0, 0), BY_VALUE, 1)                   # the interval keeps two of the four keys


def test_by_value_day_buckets_with_negative_timestamps(va):
    rng = np.random.default_rng(21)
    n = 4097
    values = rng.integers(-20 * 86400, 20 * 86400, n).astype(np.int64)
    values[:6] = [-1, 0, -86400, -86401, 86399, 86400]
    ix, m = make(va, n, 1000, values)
    with ix:
        got, n_groups, _ = same(ix, m, MATCH_ALL, BY_VALUE, 86400)
        assert n_groups == 40 and got["key"].tolist() == list(range(-20, 20)) and int(got["count"].sum()) == n
        same(ix, m, MATCH_ALL, BY_VALUE, 86400, by_count=True, limit=3)
        same(ix, m, MATCH_ALL, BY_VALUE, 1)                                      # nearly a key per row, many of them negative
        same(ix, m, MATCH_ALL, BY_VALUE, 7)


# ---------------------------------------------------------------- BY_TAG
@pytest.mark.parametrize("n", [63, 2049, 4097])
def test_by_tag(va, n):
    rng = np.random.default_rng(n)
    tags = np.zeros(n, np.uint64)
    tags[1::5] = np.uint64(1) << rng.integers(0, 64, tags[1::5].size).astype(np.uint64)
    tags[2::5] = np.uint64(1 << 63)
    tags[3::5] = np.uint64((1 << 64) - 1)
    tags[4::5] = rng.integers(0, 1 << 62, tags[4::5].size).astype(np.uint64)
    values = rng.integers(I64_MIN, I64_MAX, n, endpoint=True)
    ix, m = make(va, n, 1000, values, tags=tags)
    with ix:
        for by_count in (False, True):
            got, n_groups, n_rows = same(ix, m, MATCH_ALL, BY_TAG, by_count=by_count)
            assert n_groups == 64 and n_rows == n                                # rows without tags are considered, in no group
            assert int(got["count"].sum()) == sum(bin(int(t)).count("1") for t in tags)
        same(ix, m, (1 << 63, 0, 1, *FULL, 0, 0), BY_TAG, limit=70)
        ix.set_tags(1000, np.zeros(n, np.uint64))
        m.set_tags(1000, np.zeros(n, np.uint64))
        assert same(ix, m, MATCH_ALL, BY_TAG)[1:] == (0, n)


# ---------------------------------------------------------------- scope, predicate, offset
N = 2048 + 37


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(77)
    values = np.array([-7, -3, -1, 0, 2, 5, I64_MIN, I64_MAX], np.int64)[rng.integers(0, 8, N)]
    tags = rng.integers(0, 8, N).astype(np.uint64) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63))
    labels = np.array([0, 1, 7, 0xFFFFFFFF], np.uint32)[rng.integers(0, 4, N)]
    allow = rng.random(N) < 0.8
    dead = np.unique(np.concatenate([rng.choice(np.arange(1, N), 60, replace=False), [0, 5, 2047, 2048, N - 1]])).astype(np.uint64)
    return values, tags, labels, allow, dead


def restricted(va, world, off=1000):
    values, tags, labels, allow, dead = world
    ix, m = make(va, N, off, values, labels, tags, seed=9)
    for h in (m, ix):
        h.set_filter(allow)
        h.delete(dead + np.uint64(off))
    return ix, m


PREDS = [MATCH_ALL, (6, 1, 1 << 63, -7, 5, 1, 1), (1, 0, 0, *FULL, 0, 0), (0, 0, 0, -3, 2, 0, 0), (0, 0, 0, *FULL, 7, 1), (0, 2, 4, I64_MIN, -1, 0xFFFFFFFF, 1)]
MODES = [(BY_LABEL, None), (BY_VALUE, 1), (BY_VALUE, 3), (BY_TAG, None)]


def test_scope_predicate_and_id_offset(va, world):
    ix, m = restricted(va, world)
    with ix:
        assert ix.count_where([MATCH_ALL], True)[0] < ix.count_where([MATCH_ALL])[0] < N   # both restrictions bite
        for pred in PREDS:
            for allowed in (False, True):
                for by, width in MODES:
                    got, _, n_rows = same(ix, m, pred, by, width, allowed=allowed, what=str(pred))
                    same(ix, m, pred, by, width, by_count=True, allowed=allowed, what=str(pred))
                    assert got.size and got["first_id"].min() >= 1001            # row 0 is deleted; ids carry the offset
                    if by != BY_TAG:
                        assert int(got["count"].sum()) == n_rows == ix.count_where([pred], allowed)[0]
        got, n_groups, _ = same(ix, m, PREDS[4], BY_LABEL)                       # a predicate carrying a label: one group
        assert n_groups == 1 and got["key"].tolist() == [7]
        for pred in ((0, 1, 1, *FULL, 0, 0), (0, 0, 0, 1, 0, 0, 0)):             # unsatisfiable: zeros, and nothing is written
            for by, width in MODES:
                rc, n, groups, rows, out = raw_call(ix, pred, ORDER_COUNT, by, width or 0, 9)
                assert (rc, n, groups, rows) == (0, 0, 0, 0) and untouched(out)
                same(ix, m, pred, by, width)
        for pred in ((0, 0, 0, 6, I64_MAX - 1, 0, 0), (0, 0, 0, *FULL, 3, 1)):   # satisfiable, but no row matches
            rc, n, groups, rows, out = raw_call(ix, pred, 0, BY_LABEL, 0, 9)
            assert (rc, n, groups, rows) == (0, 0, 0, 0) and untouched(out)


def test_an_empty_handle_gives_zeros(va):
    with va.Index(DIM, "f32", "l2") as ix:
        for reserve in (0, 500):
            if reserve:
                ix.reserve(reserve)
            for flags in (0, ALLOWED, ORDER_COUNT, ALLOWED | ORDER_COUNT):
                for by, width in MODES:
                    rc, n, groups, rows, out = raw_call(ix, MATCH_ALL, flags, by, width or 0, 9)
                    assert (rc, n, groups, rows) == (0, 0, 0, 0) and untouched(out)
            got, n_groups, n_rows = ix.aggregate_where(MATCH_ALL, BY_LABEL)
            assert (got.size, n_groups, n_rows) == (0, 0, 0)


# ---------------------------------------------------------------- order, limit, optional outputs
def test_order_count_with_ties_and_limits(va):
    n = 2049
    labels = np.repeat(np.array([50, 40, 30, 20, 10, 60, 70], np.uint32), [300, 300, 300, 500, 300, 348, 1])   # four groups tie at 300
    values = np.arange(n, dtype=np.int64) - 700
    ix, m = make(va, n, 1000, values, labels)
    with ix:
        got, n_groups, _ = same(ix, m, MATCH_ALL, BY_LABEL, by_count=True)
        assert got["key"].tolist() == [20, 60, 10, 30, 40, 50, 70] and n_groups == 7
        for by_count in (False, True):
            flags = ORDER_COUNT if by_count else 0
            whole = m.aggregate_where(MATCH_ALL, BY_LABEL, None, None, flags)[0]
            for limit in (1, 6, 7, 8, 1 << 20, 0xFFFFFFFF):                      # below, at and above the group count
                rc, cnt, groups, rows, out = raw_call(ix, MATCH_ALL, flags, BY_LABEL, 0, limit, room=12)
                k = min(limit, 7)
                assert (rc, cnt, groups, rows) == (0, k, 7, n) and out[:k].tobytes() == whole[:k].tobytes() and untouched(out[k:])
                same(ix, m, MATCH_ALL, BY_LABEL, limit=min(limit, 1 << 20), by_count=by_count)
            rc, cnt, groups, rows, out = raw_call(ix, MATCH_ALL, flags, BY_LABEL, 0, 0, want=(True, True, True, False))   # limit 0, null out
            assert (rc, cnt, groups, rows) == (0, 0, 7, n)
            rc, cnt, groups, rows, out = raw_call(ix, MATCH_ALL, flags, BY_LABEL, 0, 3, want=(True, False, False, True))   # the optional counts
            assert (rc, cnt, groups, rows) == (0, 3, SENT, SENT) and out[:3].tobytes() == whole[:3].tobytes() and untouched(out[3:])


# ---------------------------------------------------------------- the group cap
def test_the_group_cap(va):
    """Exactly VROD_MAX_AGG_GROUPS distinct labels are accepted and exact; one more is VROD_ERR_CAPACITY with every output
    intact.  The rows come from add_synthetic; the model only needs their number."""
    n = MAX_AGG_GROUPS
    rng = np.random.default_rng(5)
    labels = rng.permutation(n + 1).astype(np.uint32) * np.uint32(2654435761)    # odd multiplier: distinct mod 2^32
    values = rng.integers(I64_MIN, I64_MAX, n + 1, endpoint=True)
    m = AggregateModelIndex(DIM, "bf16", "cosine")
    m.add(np.zeros((n, DIM), np.float32))
    with va.Index(DIM, "bf16", "cosine") as ix:
        ix.add_synthetic(1, 0, n)
        for h in (ix, m):
            h.set_labels(0, labels[:n])
            h.set_values(0, values[:n])
        got, n_groups, n_rows = same(ix, m, MATCH_ALL, BY_LABEL, what="at the cap")
        assert n_groups == n_rows == n and (got["count"] == 1).all()
        same(ix, m, MATCH_ALL, BY_LABEL, limit=100, by_count=True, what="at the cap")
        ix.add_synthetic(1, n, 1)
        ix.set_labels(n, labels[n:])
        before = ix.last_stats()
        for limit in (0, 4):
            rc, cnt, groups, rows, out = raw_call(ix, MATCH_ALL, 0, BY_LABEL, 0, limit)
            assert rc == ERR_CAPACITY and (cnt, groups, rows) == (SENT, SENT, SENT) and untouched(out)
        with pytest.raises(va.VrodError) as e:
            ix.aggregate_where(MATCH_ALL, BY_LABEL)
        assert e.value.code == ERR_CAPACITY and ix.last_stats() == before
        ix.delete(np.array([5], np.uint64))                                      # back under the cap: the call works again
        m.delete(np.array([5], np.uint64))
        assert ix.aggregate_where(MATCH_ALL, BY_LABEL, limit=0)[1:] == (n, n)
        assert ix.aggregate_where(MATCH_ALL, BY_VALUE, width=1 << 62, limit=0)[1:] == (4, n)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_outputs_and_stats_alone(va, world):
    import torch
    ix, m = restricted(va, world)
    rq = np.random.default_rng(12).standard_normal((2, DIM)).astype(np.float32)
    with ix:
        ix.search(rq, K)
        before = ix.last_stats()
        bad = ix._row_preds(MATCH_ALL, 1).copy()
        bad["has_label"] = 2

        def refused(code, pred=MATCH_ALL, flags=0, by=BY_LABEL, width=0, want=(True, True, True, True)):
            rc, n, groups, rows, out = raw_call(ix, pred, flags, by, width, 4, want=want)
            assert rc == code and (n, groups, rows) == (SENT, SENT, SENT) and untouched(out)

        refused(ERR_INVALID_ARG, flags=2)                                        # VROD_ORDER_DESC's bit is not a flag here
        refused(ERR_INVALID_ARG, flags=8)
        refused(ERR_INVALID_ARG, flags=2 | ORDER_COUNT | ALLOWED)
        refused(ERR_INVALID_ARG, by=3)
        refused(ERR_INVALID_ARG, by=0xFFFFFFFF)
        refused(ERR_INVALID_ARG, by=BY_VALUE, width=0)
        refused(ERR_INVALID_ARG, by=BY_VALUE, width=-1)
        refused(ERR_INVALID_ARG, by=BY_VALUE, width=I64_MIN)
        refused(ERR_INVALID_ARG, pred=bad)
        refused(ERR_INVALID_ARG, pred=None)
        refused(ERR_INVALID_ARG, want=(False, True, True, True))                 # null out_count
        refused(ERR_INVALID_ARG, want=(True, True, True, False))                 # null out, limit > 0
        assert raw_call(ix, MATCH_ALL, 0, BY_LABEL, -1, 4)[0] == 0               # width is read under BY_VALUE only
        si = torch.empty((4, K), dtype=torch.int64, device="cuda")
        ss = torch.empty((4, K), dtype=torch.float32, device="cuda")
        ix.search_begin_synthetic_device(2, 0, 4, K, si, ss)                     # a pending search
        refused(ERR_INVALID_ARG)
        with pytest.raises(va.VrodError) as e:
            ix.aggregate_where(MATCH_ALL, BY_TAG)
        assert e.value.code == ERR_INVALID_ARG
        ix.search_end()
        ix.search(rq, K)
        assert ix.last_stats() == before                                         # the same search, the same counters: nothing in between touched them
        same(ix, m, MATCH_ALL, BY_LABEL, what="after the refused calls")
        assert ix.last_stats() == before


def test_a_multi_device_handle_is_unsupported(va):
    rows = np.random.default_rng(13).standard_normal((500, DIM)).astype(np.float32)
    with va.Index(DIM, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(rows)
        for by, width in MODES:
            for limit in (0, 4):
                rc, n, groups, n_rows, out = raw_call(ix, MATCH_ALL, ORDER_COUNT, by, width or 0, limit)
                assert rc == ERR_UNSUPPORTED and (n, groups, n_rows) == (SENT, SENT, SENT) and untouched(out)
        assert (ix.count, ix.live_count()) == (500, 500)


# ---------------------------------------------------------------- determinism, and a handle that lives on
def test_repeated_calls_give_identical_bytes(va):
    rng = np.random.default_rng(14)
    n = 4097
    ix, m = make(va, n, 1000, rng.integers(I64_MIN, I64_MAX, n, endpoint=True), rng.integers(0, 900, n).astype(np.uint32),
                 rng.integers(0, 1 << 63, n).astype(np.uint64))
    with ix:
        for by, width, by_count in ((BY_LABEL, None, False), (BY_LABEL, None, True), (BY_VALUE, 1 << 55, True), (BY_TAG, None, False)):
            first = same(ix, m, MATCH_ALL, by, width, by_count=by_count, what="determinism")
            for _ in range(4):
                again = ix.aggregate_where(MATCH_ALL, by, width=width, by_count=by_count)
                assert again[0].tobytes() == first[0].tobytes() and again[1:] == first[1:]


def test_after_mutations_and_between_searches(va):
    rng = np.random.default_rng(15)
    n, off = 2300, 1000
    ix, m = make(va, n, off, rng.integers(-50, 50, n).astype(np.int64), rng.integers(0, 40, n).astype(np.uint32), rng.integers(0, 1 << 10, n).astype(np.uint64),
                 reserve=0)
    rq = rng.standard_normal((3, DIM)).astype(np.float32)
    extra = rng.standard_normal((500, DIM)).astype(np.float32)

    def all_modes(what):
        for by, width in MODES:
            same(ix, m, MATCH_ALL, by, width, what=what)
            same(ix, m, (0, 0, 512, -40, 30, 0, 0), by, width, by_count=True, what=what)

    with ix:
        ids0, sc0 = ix.search(rq, K)
        all_modes("fresh")
        ids1, sc1 = ix.search(rq, K)
        assert_same(ids1, sc1, ids0, sc0, "a search before and after an aggregation")   # the call changes nothing
        assert_same(ids1, sc1, *m.search(rq, K), "the search is the model's")
        for h in (ix, m):
            h.set_values(off + 100, np.arange(700, dtype=np.int64) * 1000 - 350_000)
        all_modes("after set_values")
        for h in (ix, m):
            h.delete(np.arange(off, off + n, 3, dtype=np.uint64))
        all_modes("after delete")
        for h in (ix, m):
            h.compact()
        assert ix.count == m.count
        all_modes("after compact")
        first_new, new_labels = off + m.count, rng.integers(30, 60, 500).astype(np.uint32)
        for h in (ix, m):
            h.add(extra)                                                         # past the reservation: the columns move
            h.set_labels(first_new, new_labels)
        all_modes("after add")
        ids2, sc2 = ix.search(rq, K)
        assert_same(ids2, sc2, *m.search(rq, K), "a search after everything")
