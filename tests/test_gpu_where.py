"""GPU tests of row values and the search with a tags + value-interval predicate per query (vrod_index_set_values /
vrod_search_where) against the CPU oracle.

The contract: query q gets, bit for bit, what the oracle returns over the rows that are live, allowed and match preds[q]
-- where_model.WhereModelIndex: scan_topk(prepared[those rows], ...), ids mapped back.  The rows are taken in ascending
order, so ties still break by the smaller id; slots beyond them are (ID_NONE, NaN).  Bit-exact: no tolerances.

The corpus is the smallest at which the grouping pass can go wrong: label_rows_per_block (256 at this size) + 37 rows, so
two blocks of the pass, the second ending in a partial 64-row wave and a partial 32-bit mask word; dim 1, 33 and 768.
"""
import numpy as np
import pytest

from index_model import ModelError
from where_model import FULL, I64_MAX, I64_MIN, WHERE_DTYPE, WhereModelIndex, as_preds, distinct_preds, unsatisfiable
from support import (  # noqa: F401
    PATH_AUTO, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, va, assert_same, row_bytes, takes_segments)

pytestmark = pytest.mark.gpu

ROWS_PER_BLOCK = 256                                 # label_plan.h label_rows_per_block(N) for N <= 2048 * 256
N = ROWS_PER_BLOCK + 37
DIMS = (1, 33, 768)
K = 10
VALUE_SET = np.array([-7, -3, -1, 0, 2, 5, I64_MIN, I64_MAX], np.int64)
ALL_ONES = 0xFFFFFFFFFFFFFFFF


def test_the_shape_is_the_one_the_pass_cuts():
    """label_plan.h label_rows_per_block, restated: whole 64-row waves, at least 256 rows."""
    rpb = max(256, ((N + 2047) // 2048 + 63) // 64 * 64)
    assert rpb == ROWS_PER_BLOCK and -(-N // rpb) == 2 and (N - rpb) % 64 and N % 32


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20264)
    corpora = {d: rng.standard_normal((N, d)).astype(np.float32) for d in DIMS + (8,)}
    queries = {d: rng.standard_normal((40, d)).astype(np.float32) for d in DIMS + (8,)}
    values = VALUE_SET[rng.integers(0, 6, N)]                                    # the small set, negatives included ...
    values[[3, 100, 255, 256, N - 1]] = I64_MIN                                  # ... and the extremes, on both sides of the block edge
    values[[4, 101, 254, 257, N - 2]] = I64_MAX
    tags = rng.integers(0, 8, N).astype(np.uint64) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63))
    allow = rng.random(N) < 0.85
    dead = rng.choice(N, 15, replace=False).astype(np.uint64)
    return corpora, queries, values, tags, allow, dead


def filled(va, world, dim, dtype, metric, restrict=False, tags=True, values=True):
    """A handle and its model with the world's rows (and tags, values; restrict: its allow list and deletions)."""
    corpora, _, vals, tg, allow, dead = world
    model = WhereModelIndex(dim, dtype, metric)
    ix = va.Index(dim, dtype, metric)
    for h in (model, ix):
        h.add(corpora[dim])
        if tags:
            h.set_tags(0, tg)
        if values:
            h.set_values(0, vals)
        if restrict:
            h.set_filter(allow)
            h.delete(dead)
    return ix, model


def unfilled(ids, sc):
    return bool((ids == ID_NONE).all() and np.isnan(sc).all())


def check_stats(st, path, dtype, dim, model, preds, k, what):
    """The counters of test_gpu_tag.check_stats: the rows of every narrow predicate, every stored row per dense one, and
    the reported path."""
    preds = as_preds(preds)
    n = model.count
    assert st["nq"] == len(preds) and st["k"] == k, f"{what}: {st}"
    rb = row_bytes(dtype, dim)
    want_bytes = want_flops = 0.0
    routes = []
    for p in distinct_preds(preds):
        if unsatisfiable(p):
            continue                                                             # in no group
        m, nqg = int(model.matching(p).size), int((preds == np.array(p, WHERE_DTYPE)).sum())
        seg = takes_segments(path, dtype, n, m, nqg, dim)
        routes.append(seg)
        want_bytes += (m if seg else n) * rb
        want_flops += 2.0 * nqg * (m if seg else n) * dim
    assert st["scan_bytes"] == want_bytes and st["scan_flops"] == want_flops, f"{what}: {st} want {want_bytes} {want_flops}"
    if all(routes):
        assert st["path"] == PATH_GATHER and st["kprime"] == 0, f"{what}: {st}"
        assert st["max_fast_err"] == 0 and st["eps_bound"] == 0 and st["fallback_queries"] == 0 and st["band_queries"] == 0, f"{what}: {st}"
    else:
        assert st["path"] != PATH_GATHER, f"{what}: {st}"
        if path != PATH_AUTO:
            assert st["path"] == path, f"{what}: {st}"
        if st["path"] != PATH_EXACT and np.isfinite(st["eps_bound"]):
            assert st["max_fast_err"] <= st["eps_bound"], f"{what}: {st}"
    return routes


# ---------------------------------------------------------------- values round trip
def test_values_round_trip(va, world):
    corpora, _, vals, _, _, _ = world
    rng = np.random.default_rng(3)
    dim, off = 33, 5000
    model = WhereModelIndex(dim, "bf16", "cosine", id_offset=off)
    with va.Index(dim, "bf16", "cosine") as ix:
        def both(name, *args):
            getattr(model, name)(*args)
            return getattr(ix, name)(*args)

        def same(what):
            got = ix.get_values(off, model.count)
            assert got.dtype == np.int64 and np.array_equal(got, model.values), what
        both("add", corpora[dim])
        ix.set_id_offset(off)
        same("0 until set")
        assert not ix.get_values(off, N).any()
        both("set_values", off + 20, vals[20:N - 20])                            # id_offset applied; a sub-range: the rest keeps 0
        same("a sub-range")
        assert ix.get_values(off + 20, 1)[0] == vals[20] and ix.get_values(off + 19, 1)[0] == 0
        both("add", rng.standard_normal((7, dim)).astype(np.float32))
        assert not ix.get_values(off + N, 7).any()                               # rows added after a set_values read 0
        same("added later")
        n = N + 7
        for first, m in ((off + n - 1, 2), (off + n + 1, 0), (off + n, 1), (off - 1, 1), (0, 1), (1 << 40, 1)):
            with pytest.raises(va.VrodError) as e:                               # not wholly within the rows: nothing changes
                ix.set_values(first, np.full(m, 9, np.int64))
            assert e.value.code == 1
            with pytest.raises(ModelError):
                model.set_values(first, np.full(m, 9, np.int64))
            with pytest.raises(va.VrodError) as e:
                ix.get_values(first, m)
            assert e.value.code == 1
        ix.set_values(off + n, np.zeros(0, np.int64))                            # n == 0 does nothing
        same("after the refused calls")
        both("set_values", off, vals)
        both("delete", (np.arange(0, n, 3) + off).astype(np.uint64))             # every third row
        both("set_values", off + 3, [I64_MIN, I64_MAX, -1])                      # deleted rows (3) may be named
        same("deleted rows named")
        live = np.flatnonzero(~model.deleted)
        both("update", (live[:50] + off).astype(np.uint64), rng.standard_normal((50, dim)).astype(np.float32))
        same("update keeps the values")
        assert np.array_equal(ix.compact(), model.compact())
        assert ix.count == model.count == n - len(range(0, n, 3))
        same("compact moves the values")
        rq = world[1][dim][:6]
        preds = [(0, 0, 0, -3, 2), (0, 0, 0, I64_MAX, I64_MAX), (0, 0, 0, *FULL), (0, 0, 0, I64_MIN, -1), (0, 0, 0, 0, 0), (0, 0, 0, -1, -1)]
        assert_same(*ix.search_where(rq, K, preds), *model.search_where(rq, K, preds), "after compact")
        both("set_values", off + 10, np.arange(-50, 50, dtype=np.int64))         # values again, on the compacted rows
        same("set_values after compact")
        assert_same(*ix.search_where(rq, K, preds), *model.search_where(rq, K, preds), "set_values after compact")


# ---------------------------------------------------------------- degenerate predicates
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_degenerate_predicates(va, world, dtype, metric):
    """A full interval leaves the tag predicate: the bits of search_tagged on the same handle.  All-zero masks as well:
    the bits of search, under the same filter and deletions."""
    _, queries, _, _, _, _ = world
    tag_preds = [(1, 0, 0), (0, 3, 0), (0, 0, 4), (1 << 63, 1, 2), (0, 0, 0), (6, 0, 1 << 63), (0, 1, 1), (0, 1 << 63, 0), (ALL_ONES, 0, 0)]
    for dim in DIMS:
        rq = queries[dim][:len(tag_preds)]
        ix, model = filled(va, world, dim, dtype, metric, restrict=True)
        with ix:
            for path in (PATH_AUTO, PATH_GATHER):
                ix.set_path(path)
                what = f"{dim}/{dtype}/{metric}/path{path}"
                ti, ts = ix.search_tagged(rq, K, np.array(tag_preds, np.uint64))
                wi, ws = ix.search_where(rq, K, [p + FULL for p in tag_preds])
                assert_same(wi, ws, ti, ts, what + " full interval == search_tagged")
                assert_same(wi, ws, *model.search_where(rq, K, [p + FULL for p in tag_preds]), what + " model")
                assert unfilled(wi[6], ws[6])                                    # all & none != 0
                pi, ps = ix.search(rq, K)
                wi, ws = ix.search_where(rq, K, [(0, 0, 0) + FULL] * len(rq))
                assert_same(wi, ws, pi, ps, what + " all-zero masks + full interval == search")
                assert_same(wi, ws, *model.search(rq, K), what + " model")


# ---------------------------------------------------------------- interval only
INTERVALS = [(-3, 2), (-7, -7), (5, 5), (-1, 0), (0, 0), (-7, -1), (2, 5),        # ends that equal stored values: both included
             (-2, 1),                                                            # spans zero, negatives present: -1 and 0, not 2
             (-6, 4), (I64_MIN, I64_MIN), (I64_MAX, I64_MAX), (I64_MIN, -7), (5, I64_MAX), (I64_MIN + 1, I64_MAX - 1), FULL,
             (6, I64_MAX - 1)]                                                   # satisfiable, no row


@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2"), ("bf16", "ip")])
def test_interval_only(va, world, dtype, metric):
    _, queries, vals, _, _, _ = world
    preds = [(0, 0, 0, lo, hi) for lo, hi in INTERVALS]
    preds[3:3] = [(0, 0, 0, 1, 0)]                                               # lo > hi and all & none != 0, mixed into the batch
    preds[9:9] = [(0, 4, 4, *FULL), (0, 0, 0, I64_MAX, I64_MIN)]
    preds += preds[:5]                                                           # repeated predicates: one group
    impossible = [q for q, p in enumerate(preds) if unsatisfiable(p)]
    assert len(impossible) == 4 and len(preds) <= 40
    # what the signed compare must see (tags play no part: the handle never set any)
    count = lambda lo, hi: int(((vals >= lo) & (vals <= hi)).sum())
    assert count(-2, 1) == int(np.isin(vals, (-1, 0)).sum()) > 0 and count(-7, -1) == int(np.isin(vals, (-7, -3, -1)).sum()) > 0
    assert count(I64_MIN, I64_MIN) == 5 and count(I64_MAX, I64_MAX) == 5 and count(6, I64_MAX - 1) == 0
    for dim in DIMS:
        rq = queries[dim][:len(preds)]
        ix, model = filled(va, world, dim, dtype, metric, tags=False)
        with ix:
            for path in (PATH_GATHER, PATH_AUTO):
                ix.set_path(path)
                what = f"{dim}/{dtype}/{metric}/path{path}"
                ids, sc = ix.search_where(rq, K, preds)
                st = ix.last_stats()
                print(what, st)
                assert_same(ids, sc, *model.search_where(rq, K, preds), what)
                check_stats(st, path, dtype, dim, model, preds, K, what)
                assert unfilled(ids[impossible], sc[impossible]), what
                for q, p in enumerate(preds):                                    # every returned row lies inside its interval
                    got = ids[q][ids[q] != ID_NONE].astype(np.int64)
                    assert ((vals[got] >= p[3]) & (vals[got] <= p[4])).all() and got.size == min(K, model.matching(p).size), (what, q)
            # a batch made only of such queries: all unfilled, no launch
            ids, sc = ix.search_where(rq[:4], K, [preds[q] for q in impossible])
            st = ix.last_stats()
            assert unfilled(ids, sc) and st["scan_launches"] == 0 and st["scan_bytes"] == 0 and st["path"] == PATH_GATHER, (dim, st)


# ---------------------------------------------------------------- tags and interval together, three routes
MIXED = [(1, 0, 0, -3, 2), (0, 3, 0, I64_MIN, 0), (0, 0, 4, -1, I64_MAX), (1 << 63, 0, 1, -7, 5), (6, 0, 0, 0, 0), (1 << 63, 1, 0, *FULL),
         (0, 0, 0, -7, 5), (0, 0, 1 << 63, 2, I64_MAX), (0, 2, 2, -7, 5), (7, 0, 0, 3, 2), (0, 0, 0, -3, 2), (1, 0, 0, -3, 2)]


@pytest.mark.parametrize("path", [PATH_GATHER, PATH_MFMA, PATH_EXACT])
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2"), ("f32", "ip")])
def test_tags_and_interval_under_a_forced_path(va, world, dtype, metric, path):
    """GATHER: every predicate scored on its own rows; MFMA, EXACT: every predicate by a masked scan (the mask kernel)."""
    _, queries, _, _, _, _ = world
    for dim in DIMS:
        rq = queries[dim][:len(MIXED)]
        ix, model = filled(va, world, dim, dtype, metric, restrict=True)
        with ix:
            ix.set_path(path)
            what = f"{dim}/{dtype}/{metric}/path{path}"
            ids, sc = ix.search_where(rq, K, MIXED)
            st = ix.last_stats()
            print(what, st)
            assert_same(ids, sc, *model.search_where(rq, K, MIXED), what)
            routes = check_stats(st, path, dtype, dim, model, MIXED, K, what)
            assert all(routes) if path == PATH_GATHER else not any(routes)
            assert unfilled(ids[8:10], sc[8:10])
            assert_same(*ix.search(rq, K), *model.search(rq, K), what + " plain search on the same handle")


@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2")])
def test_auto_routes_a_narrow_and_a_wide_predicate(va, world, dtype, metric):
    _, queries, _, _, _, _ = world
    narrow, wide = (1 << 63, 0, 0, -7, -7), (0, 0, 0, -7, 5)                     # a few rows; all but the extremes
    preds = [narrow, wide]
    for dim in DIMS:
        rq = queries[dim][:2]
        ix, model = filled(va, world, dim, dtype, metric, restrict=True)
        with ix:
            what = f"{dim}/{dtype}/{metric}/auto"
            m = [int(model.matching(p).size) for p in preds]
            assert [takes_segments(PATH_AUTO, dtype, N, m[i], 1, dim) for i in (0, 1)] == [True, False], (what, m)   # (the layout)
            ids, sc = ix.search_where(rq, K, preds)
            st = ix.last_stats()
            print(what, m, st)
            assert_same(ids, sc, *model.search_where(rq, K, preds), what)
            assert check_stats(st, PATH_AUTO, dtype, dim, model, preds, K, what) == [False, True]    # in group order: any == 0 first
            assert st["path"] != PATH_GATHER and st["scan_launches"] >= 1, (what, st)
            ids, sc = ix.search_where(rq[:1], K, [narrow])                       # the narrow one alone: its own rows only
            st = ix.last_stats()
            assert_same(ids, sc, *model.search_where(rq[:1], K, [narrow]), what + " narrow")
            assert check_stats(st, PATH_AUTO, dtype, dim, model, [narrow], K, what) == [True] and st["path"] == PATH_GATHER


# ---------------------------------------------------------------- more predicates than one pass
@pytest.mark.parametrize("path", [PATH_GATHER, PATH_AUTO])
def test_more_predicates_than_one_pass(va, world, path):
    corpora, _, _, _, _, _ = world
    rng = np.random.default_rng(43)
    dim, k, G = 8, 5, 1025                                                       # kWhereGroupsPerPass + 1
    raw = corpora[dim]
    vals = rng.integers(-40, 40, N).astype(np.int64)
    tags = rng.integers(0, 4, N).astype(np.uint64)
    rq = rng.standard_normal((G, dim)).astype(np.float32)
    pairs = [(lo, lo + w) for w in range(0, 16) for lo in range(-45, 45)][:G]     # G distinct intervals
    preds = [((j % 3 == 0) * 1, (j % 5 == 0) * 2, 0, lo, hi) for j, (lo, hi) in enumerate(pairs)]
    preds = [preds[j] for j in rng.permutation(G)]
    assert len(distinct_preds(preds)) == G and not any(unsatisfiable(p) for p in preds)
    model = WhereModelIndex(dim, "bf16", "cosine")
    with va.Index(dim, "bf16", "cosine") as ix:
        for h in (model, ix):
            h.add(raw)
            h.set_values(0, vals)
            h.set_tags(0, tags)
        ix.set_path(path)
        ids, sc = ix.search_where(rq, k, preds)
        st = ix.last_stats()
    print(path, st)
    assert_same(ids, sc, *model.search_where(rq, k, preds), f"{G} predicates path{path}")
    if path == PATH_GATHER:
        assert st["path"] == PATH_GATHER and 2 <= st["scan_launches"] <= 4, st   # one segmented launch per pass (and score chunk)


# ---------------------------------------------------------------- unfilled tails, duplicates
@pytest.mark.parametrize("path", [PATH_GATHER, PATH_AUTO, PATH_MFMA])
def test_unfilled_tails_and_ties_among_the_matching_rows(va, world, path):
    corpora, _, _, _, _, _ = world
    rng = np.random.default_rng(5)
    dim = 33
    raw = corpora[dim].copy()
    dup = [290, 7, 130, 257, 64, 200]                                            # the same vector, on both sides of the block edge
    v = rng.standard_normal(dim).astype(np.float32)
    raw[dup] = v
    vals = np.full(N, 1000, np.int64)
    vals[dup] = [10, -10, 10, 20, -10, 30]
    rq = np.stack([v, v, v, v, raw[1]])
    preds = [(0, 0, 0, 10, 10), (0, 0, 0, -10, -10), (0, 0, 0, -10, 20), (0, 0, 0, 11, 19), (0, 0, 0, 30, 999)]
    for dtype, metric in (("f32", "cosine"), ("bf16", "l2")):
        model = WhereModelIndex(dim, dtype, metric)
        with va.Index(dim, dtype, metric) as ix:
            for h in (model, ix):
                h.add(raw)
                h.set_values(0, vals)
            ix.set_path(path)
            ids, sc = ix.search_where(rq, K, preds)
        what = f"{dtype}/{metric}/path{path}"
        assert_same(ids, sc, *model.search_where(rq, K, preds), what)
        # the tie is broken by id among the matching rows only; k beyond them: an unfilled tail
        assert ids[0, :2].tolist() == [130, 290] and unfilled(ids[0, 2:], sc[0, 2:]), what
        assert ids[1, :2].tolist() == [7, 64] and unfilled(ids[1, 2:], sc[1, 2:]), what
        assert ids[2, :5].tolist() == [7, 64, 130, 257, 290] and unfilled(ids[2, 5:], sc[2, 5:]), what
        assert unfilled(ids[3], sc[3]) and ids[4, 0] == 200 and unfilled(ids[4, 1:], sc[4, 1:]), what
        assert sc[0, 0] == sc[0, 1] == sc[2, 4]


# ---------------------------------------------------------------- refusals
def test_refusals(va, world):
    import torch
    corpora, queries, vals, _, _, _ = world
    dim = 33
    raw, rq = corpora[dim], queries[dim][:8]
    preds = as_preds([(0, 0, 0, -3, 2), (1, 0, 0, *FULL)] * 4)
    with va.Index(dim, "bf16", "cosine") as ix:
        ids, sc = ix.search_where(rq, K, preds)                                  # an empty handle
        assert unfilled(ids, sc)
        ix.add(raw)
        ref = ix.search(rq, K)
        # values and tags never set: every row holds (0, 0)
        never = [(0, 0, 0, 0, 0), (0, 0, 0, -1, 1), (0, 0, 0, 1, 5), (0, 0, 0, I64_MIN, -1), (1, 0, 0, *FULL), (0, 0, 1, 0, I64_MAX), (0, 0, 0, *FULL),
                 (0, 1, 0, 0, 0)]
        ids, sc = ix.search_where(rq, K, never)
        sees = [0, 1, 5, 6]
        assert_same(ids[sees], sc[sees], ref[0][sees], ref[1][sees], "unset values: an interval that holds 0")
        assert unfilled(ids[[2, 3, 4, 7]], sc[[2, 3, 4, 7]]) and not ix.get_values(0, N).any()
        ix.set_values(0, vals)
        model = WhereModelIndex(dim, "bf16", "cosine")
        model.add(raw)
        model.set_values(0, vals)
        want = model.search_where(rq, K, preds)
        for k in (0, 3585):                                                      # k == 0, k > VROD_MAX_K
            with pytest.raises(va.VrodError) as e:
                ix.search_where(rq, k, preds)
            assert e.value.code == 1
        L, vp = ix._L, lambda a: a.ctypes.data
        oi, osc = np.zeros((8, K), np.uint64), np.zeros((8, K), np.float32)
        for args in ((None, vp(preds), vp(oi), vp(osc)), (vp(rq), None, vp(oi), vp(osc)), (vp(rq), vp(preds), None, vp(osc)),
                     (vp(rq), vp(preds), vp(oi), None)):
            assert L.vrod_search_where(ix._h, args[0], 8, K, args[1], args[2], args[3]) == 1
            assert L.vrod_search_where_device(ix._h, args[0], 8, K, args[1], args[2], args[3], None) == 1
        assert L.vrod_index_set_values(ix._h, 0, None, 4) == 1 and L.vrod_index_get_values(ix._h, 0, 4, None) == 1
        bad = rq.copy()
        bad[3, 5] = np.nan
        with pytest.raises(va.VrodError) as e:
            ix.search_where(bad, K, preds)
        assert e.value.code == 2
        assert_same(*ix.search_where(rq, K, preds), *want, "after the rejected calls")
        # a pending search blocks values and the search; after search_end both work
        dq = torch.from_numpy(rq).cuda()
        dp = torch.from_numpy(preds.view(np.int64).reshape(8, 5)).cuda()
        doi = torch.empty((8, K), dtype=torch.int64, device="cuda")
        dsc = torch.empty((8, K), dtype=torch.float32, device="cuda")
        ix.search_begin_device(dq, K, doi, dsc)
        for call in (lambda: ix.search_where(rq, K, preds), lambda: ix.set_values(0, vals[:10]), lambda: ix.search_where_device(dq, K, dp)):
            with pytest.raises(va.VrodError) as e:
                call()
            assert e.value.code == 1
        ix.search_end()
        assert_same(*ix.search_where(rq, K, preds), *want, "after search_end")
        assert np.array_equal(ix.get_values(0, N), vals)
    with va.Index(dim, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        with pytest.raises(va.VrodError) as e:
            ix.set_values(0, vals)
        assert e.value.code == 6
        oi, osc = np.full((8, K), 7, np.uint64), np.full((8, K), 7.0, np.float32)
        rc = ix._L.vrod_search_where(ix._h, rq.ctypes.data, 8, K, preds.ctypes.data, oi.ctypes.data, osc.ctypes.data)
        assert rc == 6 and (oi == 7).all() and (osc == 7.0).all()                # outputs untouched
        assert not ix.get_values(0, 100).any()


# ---------------------------------------------------------------- device form
def test_device_form_equals_host_form(va, world):
    import torch
    _, queries, _, _, _, _ = world
    dim = 768
    preds = as_preds(MIXED)
    rq = queries[dim][:len(preds)]
    ix, model = filled(va, world, dim, "bf16", "ip", restrict=True)
    with ix:
        hi, hs = ix.search_where(rq, K, preds)
        dp = torch.from_numpy(preds.view(np.int64).reshape(len(preds), 5)).cuda()
        di, ds = ix.search_where_device(torch.from_numpy(rq).cuda(), K, dp)
        assert_same(di.cpu().numpy().view(np.uint64), ds.cpu().numpy(), hi, hs, "device form")
        assert_same(hi, hs, *model.search_where(rq, K, preds), "host form")


# ---------------------------------------------------------------- one long-lived handle against the model
def sequence(rng, dim):
    """About 40 operations in mixed order; a search_where after every few.  Deterministic: everything comes from `rng`."""
    vec = lambda n: rng.standard_normal((n, dim)).astype(np.float32)
    val = lambda n: VALUE_SET[rng.integers(0, 8, n)]
    tag = lambda n: rng.integers(0, 8, n).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))
    S = ("search",)
    return [("add", vec(N)), S, ("set_values", 0, val(N)), S, ("set_tags", 0, tag(N)), S, ("delete", 0.1), S, ("set_filter", 0.8), S,
            ("update", 30), S, ("add", vec(70)), S, ("set_values", 250, val(100)), ("set_filter", 0.9), S, ("compact",), S,
            ("set_tags", 100, tag(150)), ("delete", 0.2), S, ("set_filter", None), S, ("update", 10), ("set_values", 0, val(40)), S,
            ("compact",), S, ("add", vec(300)), ("set_values", 300, val(200)), ("set_tags", 280, tag(250)), S, ("delete", 0.05),
            ("set_filter", 0.5), S, ("compact",), ("set_filter", None), S]


@pytest.mark.parametrize("dim,dtype,metric", [(33, "bf16", "cosine"), (768, "f32", "l2")])
def test_sequence(va, dim, dtype, metric):
    rng = np.random.default_rng(77)
    ops = sequence(rng, dim)
    assert 38 <= len(ops) <= 44 and {o[0] for o in ops} == {"add", "set_values", "set_tags", "delete", "update", "set_filter", "compact", "search"}
    preds = [(0, 0, 0, -3, 2), (1, 0, 0, I64_MIN, 0), (0, 2, 1, -7, 5), (1 << 63, 0, 0, *FULL), (0, 0, 0, *FULL), (0, 0, 0, 1, 0), (6, 0, 0, 5, I64_MAX),
             (0, 0, 0, -3, 2), (0, 0, 1 << 63, -1, -1)]
    rq = rng.standard_normal((len(preds), dim)).astype(np.float32)
    model = WhereModelIndex(dim, dtype, metric)
    searches = 0
    with va.Index(dim, dtype, metric) as ix:
        for step, op in enumerate(ops):
            what = f"step {step} {op[0]}"
            if op[0] == "search":
                path = (PATH_AUTO, PATH_GATHER, PATH_MFMA)[searches % 3]
                searches += 1
                ix.set_path(path)
                assert ix.count == model.count and ix.filter_count() == model.filter_count(), what
                assert np.array_equal(ix.get_values(0, model.count), model.values), what
                assert np.array_equal(ix.get_tags(0, model.count), model.tags), what
                assert_same(*ix.search_where(rq, K, preds), *model.search_where(rq, K, preds), f"{what} path{path}")
                continue
            if op[0] == "delete":                                                # a share of the live rows
                live = np.flatnonzero(~model.deleted)
                args = (rng.choice(live, max(1, int(op[1] * live.size)), replace=False).astype(np.uint64),)
            elif op[0] == "update":
                live = np.flatnonzero(~model.deleted)
                args = (rng.choice(live, op[1], replace=False).astype(np.uint64), rng.standard_normal((op[1], dim)).astype(np.float32))
            elif op[0] == "set_filter":
                args = (None if op[1] is None else rng.random(model.count) < op[1],)
            else:
                args = op[1:]
            if op[0] == "compact":
                assert np.array_equal(ix.compact(), model.compact()), what
            else:
                getattr(model, op[0])(*args)
                getattr(ix, op[0])(*args)
    assert searches >= 15
