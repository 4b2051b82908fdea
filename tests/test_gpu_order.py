"""GPU tests of ordered selection (vrod_index_select_ordered, _select_ordered_device, Index.scroll) against
order_model.OrderModelIndex, bit for bit: ids, values, count and total.

Every handle has dim 8 (the vectors matter only where a search is compared) and is reserved past its count, so rows
between the count and the capacity would show if they were ever taken.  The counts sit at the wave and work-group edges
of the passes (64 and 2048 rows, order_plan.h), the value patterns at the radix select's corners: one tie class (every
round a single bucket), only the last digit, only the first, the int64 extremes, random, and tie runs that straddle
work-group boundaries with a limit that cuts a run.
"""
import ctypes as C

import numpy as np
import pytest

from order_model import DESC, MAX_ORDERED, OrderModelIndex
from rowpred_model import ALLOWED, MATCH_ALL
from where_model import I64_MAX, I64_MIN
from support import va, assert_same  # noqa: F401

pytestmark = pytest.mark.gpu

DIM, K = 8, 10
COUNTS = [1, 63, 64, 65, 2047, 2048, 2049, 6151]
OFF = {1: 0, 63: 1000, 64: 0, 65: 1000, 2047: 0, 2048: 1000, 2049: 0, 6151: 1000}   # half of the cases carry an id offset
CYCLE = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64)
U64_MAX = (1 << 64) - 1
SENT = 0x5A5A5A5A5A5A5A5A
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 6
FULL = (I64_MIN, I64_MAX)

PATTERNS = {
    "never_set": lambda n, rng: None,
    "constant": lambda n, rng: np.full(n, -42, np.int64),
    "last_digit": lambda n, rng: rng.integers(0, 256, n).astype(np.int64),
    "first_digit": lambda n, rng: rng.integers(-128, 128, n).astype(np.int64) << np.int64(56),
    "extremes": lambda n, rng: CYCLE[np.arange(n) % CYCLE.size],
    "random": lambda n, rng: rng.integers(I64_MIN, I64_MAX, n, endpoint=True),
    "runs": lambda n, rng: np.arange(n, dtype=np.int64) // 300,
}


def make(va, n, off=0, values=None, seed=0, dtype="bf16"):
    """A handle of n rows reserved past its count, ids from `off`, and its model."""
    rng = np.random.default_rng(1000 + seed)
    rows = rng.standard_normal((n, DIM)).astype(np.float32)
    m = OrderModelIndex(DIM, dtype, "cosine", id_offset=off)
    ix = va.Index(DIM, dtype, "cosine")
    ix.reserve(n + 300)
    ix.set_id_offset(off)
    for h in (m, ix):
        if n:
            h.add(rows)
        if values is not None and n:
            h.set_values(off, values)
    return ix, m


def same(ix, m, pred, limit, desc=False, after=None, allowed=False, what=""):
    """One call equals the model: ids, values, total, and the dtypes."""
    ids, vals, total = ix.select_ordered(pred, limit, desc=desc, after=after, allowed_only=allowed)
    wi, wv, wt = m.select_ordered(pred, limit, desc, after, ALLOWED if allowed else 0)
    tag = f"{what} limit{limit} desc{desc} after{after} allowed{allowed}"
    assert ids.dtype == np.uint64 and vals.dtype == np.int64 and total == wt, f"{tag}: total {total} != {wt}"
    assert np.array_equal(ids, wi), f"{tag}: ids differ at {np.argwhere(ids != wi)[:5].ravel() if ids.shape == wi.shape else (ids.shape, wi.shape)}"
    assert np.array_equal(vals, wv), f"{tag}: values differ"
    return ids, vals, total


def raw_call(ix, pred, flags, after, limit, want_values=True, want_total=True):
    """The C entry point with sentinel-filled outputs -> (rc, count, total, ids, values)."""
    import vrod_amd
    pp = ix._row_preds(pred, 1) if not isinstance(pred, np.ndarray) else pred
    cur = None
    if after is not None:
        cur = np.zeros(1, vrod_amd.ORDER_CURSOR_DTYPE)
        cur["value"], cur["id"] = after
    room = max(min(limit, MAX_ORDERED + 8), 1) + 4
    ids, vals = np.full(room, SENT, np.uint64), np.full(room, SENT, np.int64)
    n, total = C.c_uint64(SENT), C.c_uint64(SENT)
    rc = ix._L.vrod_index_select_ordered(ix._h, pp.ctypes.data, flags, cur.ctypes.data if cur is not None else None, limit, C.byref(n),
                                         C.byref(total) if want_total else None, ids.ctypes.data, vals.ctypes.data if want_values else None)
    return rc, n.value, total.value, ids, vals


# ---------------------------------------------------------------- counts x patterns x directions x limits
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_patterns_at_the_wave_and_group_edges(va, pattern, n):
    rng = np.random.default_rng(n * 31 + len(pattern))
    ix, m = make(va, n, OFF[n], PATTERNS[pattern](n, rng), seed=n)
    limits = sorted({1, 7, 64, 65, n, n + 5})
    if pattern == "runs":                                                        # cut a tie run in the middle, on both sides of a group boundary
        limits += [x for x in (450, 2040, 2050, 2350, 4100) if x < n]
    with ix:
        assert ix.count == n
        for desc in (False, True):
            for limit in limits:
                ids, vals, total = same(ix, m, MATCH_ALL, limit, desc, what=f"{pattern} n{n}")
                assert total == n and ids.size == min(limit, n)
                if pattern in ("never_set", "constant"):                         # one tie class: the first `limit` ids
                    assert np.array_equal(ids, np.arange(min(limit, n), dtype=np.uint64) + np.uint64(OFF[n]))
            # a cursor in the middle of the listing, then one page more
            whole = m.select_ordered(MATCH_ALL, n, desc)
            mid = (int(whole[1][n // 2]), int(whole[0][n // 2]))
            _, _, total = same(ix, m, MATCH_ALL, 65, desc, after=mid, what=f"{pattern} n{n} mid")
            assert total == n - n // 2 - 1


# ---------------------------------------------------------------- scope, predicate and cursor on one restricted handle
N = 2048 + 37


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(77)
    values = np.array([-7, -3, -1, 0, 2, 5, I64_MIN, I64_MAX], np.int64)[rng.integers(0, 8, N)]
    values[0] = I64_MIN
    tags = rng.integers(0, 8, N).astype(np.uint64) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63))
    labels = np.array([0, 1, 7, 0xFFFFFFFF], np.uint32)[rng.integers(0, 4, N)]
    allow = rng.random(N) < 0.8
    dead = np.unique(np.concatenate([rng.choice(np.arange(1, N), 60, replace=False), [5, 2047, 2048, N - 1]])).astype(np.uint64)
    return values, tags, labels, allow, dead


def restricted(va, world, off=1000, row0=None):
    values, tags, labels, allow, dead = world
    values = values.copy()
    if row0 is not None:
        values[0] = row0
    ix, m = make(va, N, off, values, seed=9)
    for h in (m, ix):
        h.set_tags(off, tags)
        h.set_labels(off, labels)
        h.set_filter(allow)
        h.delete(dead + np.uint64(off))
    return ix, m


PREDS = [MATCH_ALL, (6, 1, 1 << 63, -7, 5, 1, 1), (1, 0, 0, *FULL, 0, 0), (0, 0, 0, -3, 2, 0, 0), (0, 0, 0, *FULL, 7, 1), (0, 2, 4, I64_MIN, -1, 0xFFFFFFFF, 1)]


def test_scope_and_predicate(va, world):
    ix, m = restricted(va, world)
    with ix:
        assert ix.count_where([MATCH_ALL], True)[0] < ix.count_where([MATCH_ALL])[0] < N   # both restrictions bite
        nonempty = 0
        for pred in PREDS:
            for allowed in (False, True):
                for desc in (False, True):
                    for limit in (0, 1, 64, 300, N + 5):
                        _, _, total = same(ix, m, pred, limit, desc, allowed=allowed, what=str(pred))
                        nonempty += total > 0
                    assert ix.select_ordered(pred, 0, desc=desc, allowed_only=allowed)[2] == ix.count_where([pred], allowed)[0]
                # the rows considered are select_where's
                assert np.array_equal(np.sort(ix.select_ordered(pred, N, allowed_only=allowed)[0]), ix.select_where(pred, allowed))
        assert nonempty == len(PREDS) * 4 * 5
        assert m.select_ordered(PREDS[1], N)[2] > 0                              # label, tag and interval clauses together match rows
        for pred in ((0, 1, 1, *FULL, 0, 0), (0, 0, 0, 1, 0, 0, 0)):             # unsatisfiable: zeros, and nothing is written
            rc, n, total, ids, vals = raw_call(ix, pred, DESC, None, 9)
            assert (rc, n, total) == (0, 0, 0) and (ids == SENT).all() and (vals == SENT).all()
            same(ix, m, pred, 9)
        for pred in ((0, 0, 0, 6, I64_MAX - 1, 0, 0), (0, 0, 0, *FULL, 3, 1)):   # satisfiable, but no row matches
            rc, n, total, ids, vals = raw_call(ix, pred, 0, None, 9)
            assert (rc, n, total) == (0, 0, 0) and (ids == SENT).all() and (vals == SENT).all()
            same(ix, m, pred, 9, True, allowed=True)


def test_an_empty_handle_gives_zeros(va):
    with va.Index(DIM, "f32", "l2") as ix:
        for reserve in (0, 500):
            if reserve:
                ix.reserve(reserve)
            for flags in (0, ALLOWED, DESC, ALLOWED | DESC):
                rc, n, total, ids, vals = raw_call(ix, MATCH_ALL, flags, (0, 0) if flags & DESC else None, 9)
                assert (rc, n, total) == (0, 0, 0) and (ids == SENT).all() and (vals == SENT).all()
            assert ix.select_ordered(MATCH_ALL, 0)[2] == 0 and list(ix.scroll(MATCH_ALL, 7)) == []


def test_cursors_of_every_kind(va, world):
    off = 1000
    ix, m = restricted(va, world, off)
    values, dead = world[0], world[4]
    with ix:
        live = np.flatnonzero(~m.deleted)
        inside = int(live[live.size // 2])                                       # a live row inside a large tie class
        d = int(dead[3])
        cursors = [None, (int(values[inside]), inside + off),                    # inside a tie class
                   (int(values[d]), d + off), (int(values[2048]), 2048 + off),   # a deleted row's own (value, id)
                   (2, 7), (2, off - 1), (2, 0),                                 # ids below the offset: the whole class is still ahead
                   (2, off + N), (2, off + N + 299), (2, off + N + 100000),      # at and beyond the count, within and past the capacity
                   (2, U64_MAX), (-1, U64_MAX), (I64_MIN, U64_MAX), (I64_MAX, U64_MAX),   # the whole tie class is skipped
                   (1, 12), (3, 0), (-100, off + 5),                             # a value no row carries
                   (I64_MIN, 0), (I64_MAX, 0), (I64_MIN, off), (I64_MAX, off)]
        for after in cursors:
            for desc in (False, True):
                for allowed in (False, True):
                    for limit in (0, 5, N):
                        same(ix, m, MATCH_ALL, limit, desc, after, allowed, "cursor")
                same(ix, m, PREDS[3], 50, desc, after, False, "cursor+pred")
        # inside a tie class: equal value and smaller id out, larger id in
        v = int(values[inside])
        ids, vals, _ = ix.select_ordered(MATCH_ALL, N, after=(v, inside + off))
        tied = ids[vals == v]
        assert tied.size and tied.min() > inside + off and (vals >= v).all()
        every = ix.select_ordered(MATCH_ALL, N)
        assert np.array_equal(tied, every[0][(every[1] == v) & (every[0] > inside + off)])
        # UINT64_MAX skips the whole class
        ids, vals, _ = ix.select_ordered(MATCH_ALL, N, after=(v, U64_MAX))
        assert (vals > v).all() and ids.size == int((every[1] > v).sum())
        # past the end: nothing is left, in either direction
        assert ix.select_ordered(MATCH_ALL, 5, after=(I64_MAX, U64_MAX))[2] == 0
        assert ix.select_ordered(MATCH_ALL, 5, desc=True, after=(I64_MIN, U64_MAX))[2] == 0
        last = (int(every[1][-1]), int(every[0][-1]))
        assert ix.select_ordered(MATCH_ALL, 5, after=last)[2] == 0 and ix.select_ordered(MATCH_ALL, 5, after=(last[0], last[1] - 1))[2] == 1


@pytest.mark.parametrize("desc,row0", [(False, I64_MIN), (True, I64_MAX), (False, 0), (True, 0)])
def test_the_first_possible_cursor_leaves_out_only_row_zero(va, world, desc, row0):
    """(INT64_MIN, 0) ascending and (INT64_MAX, 0) descending are before every row but id 0 carrying that value."""
    ix, m = restricted(va, world, off=0, row0=row0)
    with ix:
        assert not m.deleted[0]
        first = (I64_MAX if desc else I64_MIN, 0)
        ids, _, total = same(ix, m, MATCH_ALL, N, desc, first, what="first cursor")
        every = ix.select_ordered(MATCH_ALL, N, desc=desc)
        gone = row0 == first[0]
        assert total == every[2] - int(gone)
        assert np.array_equal(ids, every[0][1:] if gone else every[0]) and (every[0][0] == 0) == gone


# ---------------------------------------------------------------- paging
def test_scroll_concatenates_to_the_one_call_result(va):
    rng = np.random.default_rng(3)
    ix, m = make(va, 300, 1000, PATTERNS["last_digit"](300, rng))
    with ix:
        for desc in (False, True):
            whole = same(ix, m, MATCH_ALL, 300, desc, what="whole")
            pages = list(ix.scroll(MATCH_ALL, 7, desc=desc))
            assert len(pages) == -(-300 // 7) and all(p[0].size == 7 for p in pages[:-1])
            assert np.array_equal(np.concatenate([p[0] for p in pages]), whole[0]) and np.array_equal(np.concatenate([p[1] for p in pages]), whole[1])
        pred = (0, 0, 0, 10, 99, 0, 0)
        assert np.array_equal(np.concatenate([p[0] for p in ix.scroll(pred, 7)]), m.select_ordered(pred, 300)[0])
        assert list(ix.scroll((0, 0, 0, 1, 0, 0, 0), 7)) == []


@pytest.mark.parametrize("desc", [False, True])
def test_pages_stay_exact_under_mutation(va, desc):
    """A deletion, an add, a set_values on a row not yet visited and a compact between pages: the library and the model,
    stepped the same way, give the same pages."""
    rng = np.random.default_rng(4)
    off = 1000
    ix, m = make(va, 300, off, PATTERNS["last_digit"](300, rng))
    extra, more = rng.standard_normal((20, DIM)).astype(np.float32), rng.integers(0, 256, 20).astype(np.int64)
    with ix:
        got, want = ix.scroll(MATCH_ALL, 7, desc=desc), m.scroll(MATCH_ALL, 7, desc)
        seen, n_pages = [], 0
        while True:
            a, b = next(got, None), next(want, None)
            assert (a is None) == (b is None), f"page {n_pages}"
            if a is None:
                break
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"page {n_pages}"
            seen.append(a[0])
            n_pages += 1
            live = np.flatnonzero(~m.deleted) + m.offset
            visited = np.concatenate(seen)
            ahead = np.setdiff1d(live, visited)
            if n_pages == 3:                                                     # delete rows behind and ahead of the cursor
                gone = np.concatenate([visited[:4], ahead[:6]]).astype(np.uint64)
                for h in (ix, m):
                    h.delete(gone)
            elif n_pages == 6:                                                   # new rows, with values on both sides of the cursor
                for h in (ix, m):
                    h.add(extra)
                    h.set_values(off + 300, more)
            elif n_pages == 9:                                                   # a row not yet visited moves to the far end
                target = int(ahead[ahead.size // 2])
                for h in (ix, m):
                    h.set_values(target, np.array([-5 if desc else 300], np.int64))
            elif n_pages == 12:                                                  # compact: ids change under the cursor
                for h in (ix, m):
                    h.compact()
                assert ix.count == m.count
                seen = []                                                        # old ids mean nothing any more
        assert n_pages > 30


# ---------------------------------------------------------------- limits
@pytest.fixture(scope="module")
def big(va):
    n = 70_001
    rng = np.random.default_rng(70)
    values = PATTERNS["random"](n, rng)
    ix, m = make(va, n, 1000, values, seed=70)
    yield ix, m, n
    ix.close()


def test_the_largest_limit_takes_the_large_sort(va, big):
    ix, m, n = big
    for desc in (False, True):
        ids, _, total = same(ix, m, MATCH_ALL, MAX_ORDERED, desc, what="max")
        assert ids.size == MAX_ORDERED and total == n
    same(ix, m, (0, 0, 0, -(1 << 62), 1 << 62, 0, 0), MAX_ORDERED, True, after=(1 << 61, 0), what="max, pred and cursor")
    for limit in (2048, 2049, 4096, 4097, 40_000):                               # every size of the sort, and the tile's edge
        same(ix, m, MATCH_ALL, limit, what="sort sizes")


def test_limit_beyond_the_maximum_is_refused_and_zero_counts(va, big):
    ix, m, n = big
    before = ix.last_stats()
    rc, cnt, total, ids, vals = raw_call(ix, MATCH_ALL, 0, None, MAX_ORDERED + 1)
    assert rc == ERR_INVALID_ARG and cnt == SENT and total == SENT and (ids == SENT).all() and (vals == SENT).all()
    with pytest.raises(ValueError):
        ix.select_ordered(MATCH_ALL, MAX_ORDERED + 1)
    pp = ix._row_preds(MATCH_ALL, 1)
    cnt, total = C.c_uint64(SENT), C.c_uint64(SENT)
    assert ix._L.vrod_index_select_ordered(ix._h, pp.ctypes.data, DESC, None, 0, C.byref(cnt), C.byref(total), None, None) == 0   # count only
    assert (cnt.value, total.value) == (0, n)
    assert ix._L.vrod_index_select_ordered_device(ix._h, pp.ctypes.data, 0, None, 0, C.byref(cnt), C.byref(total), None, None, None) == 0
    assert (cnt.value, total.value) == (0, n)
    assert ix.last_stats() == before


# ---------------------------------------------------------------- outputs
def test_optional_outputs_and_untouched_tails(va, world):
    ix, m = restricted(va, world)
    with ix:
        wi, wv, wt = m.select_ordered(PREDS[3], 40, True)
        rc, n, total, ids, vals = raw_call(ix, PREDS[3], DESC, None, 40)
        assert (rc, n, total) == (0, 40, wt) and np.array_equal(ids[:40], wi) and np.array_equal(vals[:40], wv)
        assert (ids[40:] == SENT).all() and (vals[40:] == SENT).all()            # entries past the count keep the sentinel
        rc, n, total, ids, vals = raw_call(ix, PREDS[3], DESC, None, 40, want_values=False)
        assert (rc, n, total) == (0, 40, wt) and np.array_equal(ids[:40], wi) and (vals == SENT).all()
        rc, n, total, ids, vals = raw_call(ix, PREDS[3], DESC, None, 40, want_total=False)
        assert (rc, n, total) == (0, 40, SENT) and np.array_equal(ids[:40], wi) and np.array_equal(vals[:40], wv)
        wi, wv, wt = m.select_ordered(PREDS[5], 500)                             # fewer rows than the limit
        assert 0 < wt < 500
        rc, n, total, ids, vals = raw_call(ix, PREDS[5], 0, None, 500)
        assert (rc, n, total) == (0, wt, wt) and np.array_equal(ids[:wt], wi) and (ids[wt:] == SENT).all() and (vals[wt:] == SENT).all()


def test_the_device_form_writes_the_same_bytes(va, world):
    import torch
    ix, m = restricted(va, world)
    with ix:
        stream = torch.cuda.Stream()
        for desc, after, limit in ((False, None, 300), (True, (2, 1500), 2300), (False, (0, U64_MAX), 64)):
            wi, wv, wt = m.select_ordered(MATCH_ALL, limit, desc, after, ALLOWED)
            with torch.cuda.stream(stream):
                oi = torch.full((limit + 3,), SENT, dtype=torch.int64, device="cuda")   # written on the caller's stream, just before
                ov = torch.full((limit + 3,), SENT, dtype=torch.int64, device="cuda")
                n, total, oi, ov = ix.select_ordered_device(MATCH_ALL, limit, desc=desc, after=after, allowed_only=True, out_ids=oi, out_values=ov)
            hi, hv = oi.cpu().numpy(), ov.cpu().numpy()
            assert (n, total) == (wi.size, wt)
            assert np.array_equal(hi[:n].view(np.uint64), wi) and np.array_equal(hv[:n], wv)
            assert (hi[n:] == SENT).all() and (hv[n:] == SENT).all()
            host = ix.select_ordered(MATCH_ALL, limit, desc=desc, after=after, allowed_only=True)
            assert hi[:n].tobytes() == host[0].tobytes() and hv[:n].tobytes() == host[1].tobytes()
        n, total, oi, ov = ix.select_ordered_device(MATCH_ALL, 10)               # tensors of its own
        assert n == 10 and oi.dtype == torch.int64 and np.array_equal(oi.cpu().numpy().view(np.uint64), m.select_ordered(MATCH_ALL, 10)[0])
        pp = ix._row_preds(MATCH_ALL, 1)
        cnt = C.c_uint64(SENT)
        assert ix._L.vrod_index_select_ordered_device(ix._h, pp.ctypes.data, 0, None, 5, C.byref(cnt), None, oi.data_ptr(), None, None) == 0   # no values, no total
        assert cnt.value == 5


def test_ordered_ids_feed_a_candidate_search(va, world):
    """Most similar among the 500 rows with the largest values: the ids never leave the device."""
    import torch
    ix, m = restricted(va, world)
    rq = np.random.default_rng(11).standard_normal((4, DIM)).astype(np.float32)
    with ix:
        n, total, ids, _ = ix.select_ordered_device(PREDS[2], 500, desc=True)
        assert n == 500 < total
        lims = (torch.arange(5, dtype=torch.int32, device="cuda") * n).contiguous()
        oi, osc = ix.search_candidates_device(torch.from_numpy(rq).cuda(), K, lims, ids[:n].repeat(4).contiguous())
        rows = np.sort(m.select_ordered(PREDS[2], 500, True)[0].astype(np.int64) - m.offset)
        rows = rows[m.eligible()[rows]]                                          # a candidate search honours the filter
        assert rows.size > K
        assert_same(oi.cpu().numpy().view(np.uint64), osc.cpu().numpy(), *m._topk(rows, m._queries(rq), K), "candidates")


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
        oi = torch.full((8,), SENT, dtype=torch.int64, device="cuda")
        ov = torch.full((8,), SENT, dtype=torch.int64, device="cuda")

        def refused(code, pred=MATCH_ALL, flags=0):
            rc, n, total, ids, vals = raw_call(ix, pred, flags, (0, 0), 4)
            assert rc == code and n == SENT and total == SENT and (ids == SENT).all() and (vals == SENT).all()
            pp = pred if isinstance(pred, np.ndarray) else ix._row_preds(pred, 1)
            cnt, tot = C.c_uint64(SENT), C.c_uint64(SENT)
            assert ix._L.vrod_index_select_ordered_device(ix._h, pp.ctypes.data, flags, None, 4, C.byref(cnt), C.byref(tot), oi.data_ptr(), ov.data_ptr(),
                                                          None) == code
            assert cnt.value == SENT and tot.value == SENT and (oi.cpu() == SENT).all() and (ov.cpu() == SENT).all()

        refused(ERR_INVALID_ARG, flags=4)
        refused(ERR_INVALID_ARG, flags=4 | DESC | ALLOWED)
        refused(ERR_INVALID_ARG, flags=0x80000000)
        refused(ERR_INVALID_ARG, pred=bad)
        pp = ix._row_preds(MATCH_ALL, 1)
        cnt = C.c_uint64(SENT)
        assert ix._L.vrod_index_select_ordered(ix._h, None, 0, None, 4, C.byref(cnt), None, oi.data_ptr(), None) == ERR_INVALID_ARG   # null pred
        assert ix._L.vrod_index_select_ordered(ix._h, pp.ctypes.data, 0, None, 4, None, None, oi.data_ptr(), None) == ERR_INVALID_ARG   # null out_count
        assert ix._L.vrod_index_select_ordered(ix._h, pp.ctypes.data, 0, None, 4, C.byref(cnt), None, None, None) == ERR_INVALID_ARG    # null out_ids, limit > 0
        assert cnt.value == SENT
        si = torch.empty((4, K), dtype=torch.int64, device="cuda")
        ss = torch.empty((4, K), dtype=torch.float32, device="cuda")
        ix.search_begin_synthetic_device(2, 0, 4, K, si, ss)                     # a pending search
        refused(ERR_INVALID_ARG)
        with pytest.raises(va.VrodError) as e:
            next(ix.scroll(MATCH_ALL, 7))
        assert e.value.code == ERR_INVALID_ARG
        ix.search_end()
        ix.search(rq, K)
        assert ix.last_stats() == before                                         # the same search, the same counters: nothing in between touched them
        same(ix, m, MATCH_ALL, 4, after=(0, 0), what="after the refused calls")
        assert ix.last_stats() == before


def test_a_multi_device_handle_is_unsupported(va):
    rows = np.random.default_rng(13).standard_normal((500, DIM)).astype(np.float32)
    with va.Index(DIM, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(rows)
        pp = ix._row_preds(MATCH_ALL, 1)
        ids, vals = np.full(8, SENT, np.uint64), np.full(8, SENT, np.int64)
        n, total = C.c_uint64(SENT), C.c_uint64(SENT)
        L = ix._L
        assert L.vrod_index_select_ordered(ix._h, pp.ctypes.data, DESC, None, 4, C.byref(n), C.byref(total), ids.ctypes.data, vals.ctypes.data) == ERR_UNSUPPORTED
        assert L.vrod_index_select_ordered_device(ix._h, pp.ctypes.data, 0, None, 0, C.byref(n), C.byref(total), None, None, None) == ERR_UNSUPPORTED
        assert n.value == SENT and total.value == SENT and (ids == SENT).all() and (vals == SENT).all()
        assert (ix.count, ix.live_count()) == (500, 500)


# ---------------------------------------------------------------- determinism
def test_repeated_calls_give_identical_bytes(va):
    rng = np.random.default_rng(14)
    ix, m = make(va, 6151, 1000, PATTERNS["last_digit"](6151, rng))
    with ix:
        for desc, limit in ((False, 1000), (True, 3000), (False, 6151)):
            first = same(ix, m, MATCH_ALL, limit, desc, what="determinism")
            for _ in range(4):
                again = ix.select_ordered(MATCH_ALL, limit, desc=desc)
                assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes() and again[2] == first[2]
