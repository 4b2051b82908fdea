"""GPU tests of the row-predicate operations (vrod_index_count_where, _select_where, _delete_where, _set_filter_where,
_set_tags_where) against rowpred_model.RowPredModelIndex, which expresses each of them through the id-based calls.

The corpus is the smallest at which the pass can go wrong: kRowPredRowsPerGroup (2048) + 37 rows, so two work-groups, a
last wave that is partial and a last mask word that is partial, added after reserve(N + 300) so that the capacity exceeds
the count.  The vectors matter only where a search is compared: dim 8, and 33 once.  Everything is exact: counts, ids and,
for the searches, ids and score bits (support.assert_same).
"""
import ctypes as C

import numpy as np
import pytest

from rowpred_model import ALLOWED, MATCH_ALL, ROWPRED_DTYPE, RowPredModelIndex
from where_model import I64_MAX, I64_MIN
from support import PATH_AUTO, PATH_EXACT, PATH_GATHER, ID_NONE, va, assert_same, bits  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS_PER_GROUP = 2048                                # rowpred_plan.h kRowPredRowsPerGroup
PREDS_PER_PASS = 1024                                # rowpred_plan.h kRowPredsPerPass
N = ROWS_PER_GROUP + 37
DIM, K, OFF = 8, 10, 5000
VALUE_SET = np.array([-7, -3, -1, 0, 2, 5, I64_MIN, I64_MAX], np.int64)      # the value set of test_gpu_where.py
LABEL_SET = np.array([0, 1, 7, 0xFFFFFFFF], np.uint32)
B63 = 1 << 63
FULL = (I64_MIN, I64_MAX)
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_CAPACITY = 1, 6, 8

GRID = [
    MATCH_ALL,
    (1, 0, 0, *FULL, 0, 0), (0, 3, 0, *FULL, 0, 0), (0, 0, 4, *FULL, 0, 0), (B63, 0, 0, *FULL, 0, 0), (0, B63, 0, *FULL, 0, 0), (0, 0, B63, *FULL, 0, 0),
    (0, 0, 0, -3, 2, 0, 0), (0, 0, 0, I64_MIN, I64_MIN, 0, 0), (0, 0, 0, I64_MAX, I64_MAX, 0, 0), (0, 0, 0, I64_MIN, -1, 0, 0),
    (0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 5, I64_MAX, 0, 0), (0, 0, 0, I64_MIN + 1, I64_MAX - 1, 0, 0),
    (0, 0, 0, *FULL, 0, 1), (0, 0, 0, *FULL, 1, 1), (0, 0, 0, *FULL, 7, 1), (0, 0, 0, *FULL, 0xFFFFFFFF, 1),
    (0, 0, 0, *FULL, 7, 0),                                                      # a label that is not compared
    (6, 1, B63, -7, 5, 0, 0), (6, 1, B63, -7, 5, 1, 1), (B63 | 1, 0, 2, -1, I64_MAX, 0xFFFFFFFF, 1), (7, 0, 0, -3, 2, 7, 1),   # all together
    (0, 0, 0, 0, 0, 0, 1),                                                       # accepts 0 everywhere: all rows of a handle without columns
    (0, 1, 1, *FULL, 0, 0), (0, 0, 0, 1, 0, 0, 0), (0, B63, B63, 5, 4, 7, 1),    # unsatisfiable
    (0, 0, 0, 6, I64_MAX - 1, 0, 0), (0, 0, 0, *FULL, 3, 1),                     # satisfiable, no row
]


def test_the_shape_is_the_one_the_pass_cuts():
    """rowpred_plan.h restated: 2048 rows per work-group, whole 64-row waves."""
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vrod_amd", "csrc", "rowpred_plan.h")).read()
    assert f"constexpr uint32_t kRowPredRowsPerGroup = {ROWS_PER_GROUP};" in text and f"constexpr uint32_t kRowPredsPerPass = {PREDS_PER_PASS};" in text
    assert ROWS_PER_GROUP % 64 == 0 and -(-N // ROWS_PER_GROUP) == 2 and (N - ROWS_PER_GROUP) % 64 and N % 32
    assert -(-(N + 300) // 256) * 256 > N + 64                                   # the capacity reaches past the last wave


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20265)
    corpora = {d: rng.standard_normal((N, d)).astype(np.float32) for d in (DIM, 33)}
    queries = {d: rng.standard_normal((12, d)).astype(np.float32) for d in (DIM, 33)}
    values = VALUE_SET[rng.integers(0, 6, N)]                                    # the small set, negatives included ...
    values[[3, 100, ROWS_PER_GROUP - 1, ROWS_PER_GROUP, N - 1]] = I64_MIN        # ... and the extremes, on both sides of the work-group edge
    values[[4, 101, ROWS_PER_GROUP - 2, ROWS_PER_GROUP + 1, N - 2]] = I64_MAX
    tags = rng.integers(0, 8, N).astype(np.uint64) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63))
    labels = LABEL_SET[rng.integers(0, 4, N)]
    allow = rng.random(N) < 0.8
    dead = rng.choice(N, 60, replace=False).astype(np.uint64)
    return corpora, queries, values, tags, labels, allow, dead


def filled(va, world, dim=DIM, dtype="bf16", metric="cosine", restrict=False, tags=True, values=True, labels=True, off=0):
    """A handle and its model with the world's rows and columns (restrict: its allow list and deletions), ids from `off`."""
    corpora, _, vals, tg, lab, allow, dead = world
    model = RowPredModelIndex(dim, dtype, metric, id_offset=off)
    ix = va.Index(dim, dtype, metric)
    ix.reserve(N + 300)
    ix.set_id_offset(off)
    for h in (model, ix):
        h.add(corpora[dim])
        if tags:
            h.set_tags(off, tg)
        if values:
            h.set_values(off, vals)
        if labels:
            h.set_labels(off, lab)
        if restrict:
            h.set_filter(allow)
            h.delete(dead + np.uint64(off))
    return ix, model


def same_state(ix, model, what):
    assert (ix.count, ix.live_count(), ix.filter_count()) == (model.count, model.live_count(), model.filter_count()), what
    for flags in (0, ALLOWED):
        assert np.array_equal(ix.select_where(MATCH_ALL, bool(flags)), model.select_where(MATCH_ALL, flags)), what


def same_searches(ix, model, rq, what, paths=(PATH_AUTO, PATH_GATHER, PATH_EXACT)):
    for path in paths:
        ix.set_path(path)
        assert_same(*ix.search(rq, K), *model.search(rq, K), f"{what} path{path}")
    ix.set_path(PATH_AUTO)


# ---------------------------------------------------------------- count and select
STATES = {"fresh": {}, "restricted": dict(restrict=True, off=OFF), "no_tags": dict(tags=False, restrict=True), "no_values": dict(values=False),
          "no_labels": dict(labels=False, off=OFF), "no_columns": dict(tags=False, values=False, labels=False, restrict=True)}


@pytest.mark.parametrize("state", list(STATES))
def test_count_and_select_equal_the_model(va, world, state):
    ix, model = filled(va, world, **STATES[state])
    with ix:
        nonempty = 0
        for flags in (0, ALLOWED):
            want = [model.select_where(p, flags) for p in GRID]
            got = ix.count_where(GRID, bool(flags))
            print(state, flags, got.tolist())
            assert got.dtype == np.uint64 and got.tolist() == [w.size for w in want], f"{state} flags{flags}"
            for p, w in zip(GRID, want):
                ids = ix.select_where(p, bool(flags))
                assert ids.dtype == np.uint64 and np.array_equal(ids, w), f"{state} flags{flags} {p}"
                assert ix.count_where([p], bool(flags))[0] == w.size              # a table of one
            nonempty += sum(w.size > 0 for w in want)
            assert all(w.size == 0 for w in want[-5:])
        assert nonempty >= (20 if state != "no_columns" else 8)
        # match-all returns exactly the rows below the count, never one of the reserved tail
        every = ix.select_where(MATCH_ALL)
        assert every.size == model.live_count() and int(every[-1]) < model.offset + N and np.all(np.diff(every.astype(np.int64)) > 0)
        if state == "no_columns":                                                # a predicate that accepts 0 matches every row
            assert ix.count_where([GRID[23]])[0] == model.live_count() and ix.count_where([GRID[23]], True)[0] == model.filter_count()
        if STATES[state].get("restrict"):
            assert ix.count_where([MATCH_ALL], True)[0] == model.filter_count() < ix.count_where([MATCH_ALL])[0] == model.live_count() < N
        assert ix.count_where([]).size == 0
    with va.Index(DIM, "f32", "l2") as empty:                                    # an empty handle gives zeros
        assert empty.count_where(GRID).tolist() == [0] * len(GRID) and empty.select_where(MATCH_ALL).size == 0
        empty.reserve(500)
        assert empty.count_where(GRID, True).tolist() == [0] * len(GRID) and empty.select_where(MATCH_ALL).size == 0


def test_count_with_more_predicates_than_one_pass(va, world):
    ix, model = filled(va, world, restrict=True, off=OFF)
    distinct = [(a, 0, c, lo, hi, lab, has) for a in (0, 1, 6, B63) for c in (0, 2) for lo in (I64_MIN, -7, -3, -1, 0, 2) for hi in (-1, 0, 2, 5, I64_MAX)
                for lab, has in ((0, 0), (0, 1), (1, 1), (7, 1), (0xFFFFFFFF, 1))]
    assert len(set(distinct)) == len(distinct) == 1200 > PREDS_PER_PASS and sum(p[3] <= p[4] for p in distinct) > PREDS_PER_PASS
    rng = np.random.default_rng(9)
    preds = [distinct[i] for i in rng.permutation(len(distinct))] + [distinct[i] for i in rng.integers(0, len(distinct), 150)] + [MATCH_ALL] * 3
    with ix:
        for flags in (0, ALLOWED):
            got = ix.count_where(np.array(preds, ROWPRED_DTYPE), bool(flags))
            want = model.count_where(preds, flags)
            assert np.array_equal(got, want), f"flags{flags}: {np.flatnonzero(got != want)[:5]}"
            assert (want > 0).sum() > 600 and want[-1] == (model.filter_count() if flags else model.live_count())
        exact = [p for p in distinct if p[3] <= p[4]][:PREDS_PER_PASS + 1]        # one past a full table: a second pass of one
        assert len(exact) == PREDS_PER_PASS + 1
        assert np.array_equal(ix.count_where(exact[:PREDS_PER_PASS]), model.count_where(exact[:PREDS_PER_PASS]))
        assert np.array_equal(ix.count_where(exact), model.count_where(exact))


def test_select_capacity_contract(va, world):
    ix, model = filled(va, world, restrict=True, off=OFF)
    L = None
    with ix:
        L = ix._L
        for p in (GRID[7], GRID[16], MATCH_ALL):
            want = model.select_where(p, ALLOWED)
            m = want.size
            assert m > 2
            pp = ix._row_preds(p, 1)
            n = C.c_uint64(99)
            rc = L.vrod_index_select_where(ix._h, pp.ctypes.data, 1, 0, C.byref(n), None)     # the count-only form
            assert rc == ERR_CAPACITY and n.value == m
            buf = np.full(m + 3, 0x7777, np.uint64)
            n = C.c_uint64(99)
            rc = L.vrod_index_select_where(ix._h, pp.ctypes.data, 1, m - 1, C.byref(n), buf.ctypes.data)
            assert rc == ERR_CAPACITY and n.value == m                           # one short: the count is exact
            with pytest.raises(va.VrodError) as e:
                ix.select_where(p, True, capacity=m - 1)
            assert e.value.code == ERR_CAPACITY and e.value.count == m
            buf[:] = 0x7777
            rc = L.vrod_index_select_where(ix._h, pp.ctypes.data, 1, m, C.byref(n), buf.ctypes.data)
            assert rc == 0 and n.value == m and np.array_equal(buf[:m], want) and (buf[m:] == 0x7777).all()   # the sentinel stays
            assert np.all(np.diff(buf[:m].astype(np.int64)) > 0)                 # strictly ascending
            assert np.array_equal(ix.select_where(p, True, capacity=m + 100), want)
        n = C.c_uint64(99)
        none = ix._row_preds(GRID[25], 1)                                        # nothing matches: the count-only form is VROD_OK
        assert L.vrod_index_select_where(ix._h, none.ctypes.data, 0, 0, C.byref(n), None) == 0 and n.value == 0
        assert L.vrod_index_select_where(ix._h, none.ctypes.data, 0, 4, C.byref(n), None) == ERR_INVALID_ARG   # a capacity needs a buffer
        assert L.vrod_index_select_where(ix._h, none.ctypes.data, 0, 0, None, None) == ERR_INVALID_ARG


def test_select_device_form_feeds_a_candidate_search(va, world):
    import torch
    _, queries, *_ = world
    ix, model = filled(va, world, restrict=True, off=OFF)
    rq = queries[DIM][:4]
    with ix:
        for p, flags in ((GRID[7], ALLOWED), (GRID[16], 0), (MATCH_ALL, ALLOWED), (GRID[25], 0)):
            want = model.select_where(p, flags)
            m = want.size
            out = torch.full((m + 5,), 0x7777, dtype=torch.int64, device="cuda")
            rc, n, ids = ix.select_where_device(p, m, bool(flags), out_ids=out)
            assert rc == 0 and n == m and ids is out
            host = out.cpu().numpy().view(np.uint64)
            assert np.array_equal(host[:m], want) and (host[m:] == 0x7777).all()
            if m:
                rc, n, _ = ix.select_where_device(p, m - 1, bool(flags))
                assert rc == ERR_CAPACITY and n == m
                rc, n, _ = ix.select_where_device(p, 0, bool(flags))
                assert rc == ERR_CAPACITY and n == m
        # the ids of the device form, as they are, as every query's candidate list
        p = GRID[7]
        rows = model.matching(p, ALLOWED)
        rc, n, ids = ix.select_where_device(p, rows.size, True)
        assert rc == 0 and n == rows.size
        lims = torch.zeros(2, dtype=torch.int32, device="cuda")
        lims[1] = n
        oi, osc = ix.search_candidates_device(torch.from_numpy(rq[:1]).cuda(), K, lims, ids[:n].contiguous())
        assert_same(oi.cpu().numpy().view(np.uint64), osc.cpu().numpy(), *model._topk(rows, model._queries(rq[:1]), K), "candidates")
        keys = ix.ids_to_keys_device(ids[:n].contiguous())                       # accepted; no keys on this handle
        assert (keys.cpu().numpy().view(np.uint64) == ID_NONE).all()


# ---------------------------------------------------------------- delete_where
@pytest.mark.parametrize("dim,dtype,metric", [(DIM, "bf16", "cosine"), (33, "f32", "l2")])
def test_delete_where(va, world, dim, dtype, metric):
    _, queries, *_ = world
    rq = queries[dim]
    ix, model = filled(va, world, dim, dtype, metric, restrict=True, off=OFF)
    with ix:
        same_searches(ix, model, rq, "before")                                   # the same queries before and after: a stale mask would show
        p = (0, 0, 0, -3, I64_MAX, 7, 1)
        under_filter, all_live = model.matching(p, ALLOWED).size, model.matching(p, 0).size
        assert 0 < under_filter < all_live
        assert ix.delete_where(p, allowed_only=True) == model.delete_where(p, ALLOWED) == under_filter   # exact under the filter
        same_state(ix, model, "delete_where under the filter")
        same_searches(ix, model, rq, "after delete_where under the filter")
        assert ix.delete_where(p, allowed_only=True) == 0                        # again: nothing left to die
        left = all_live - under_filter
        assert ix.delete_where(p) == model.delete_where(p, 0) == left > 0        # the rows the filter hid
        same_state(ix, model, "delete_where")
        same_searches(ix, model, rq, "after delete_where")
        assert ix.delete_where(p) == 0 and ix.delete_where(GRID[24]) == 0 and ix.delete_where(GRID[27]) == 0
        same_state(ix, model, "deletes of nothing")
        ix.set_filter(None)
        model.set_filter(None)
        for q in (GRID[8], GRID[4]):                                             # INT64_MIN on both sides of the edge; bit 63
            assert ix.delete_where(q) == model.delete_where(q, 0) > 0
            same_state(ix, model, f"delete_where {q}")
        same_searches(ix, model, rq, "without the filter")
        assert np.array_equal(ix.compact(), model.compact())                     # the survivors
        same_state(ix, model, "compact")
        assert np.array_equal(ix.get_values(OFF, model.count), model.values) and np.array_equal(ix.get_labels(OFF, model.count), model.labels)
        same_searches(ix, model, rq, "after compact")
        assert ix.delete_where(MATCH_ALL) == model.delete_where(MATCH_ALL, 0) == model.count
        same_state(ix, model, "everything deleted")
        ids, sc = ix.search(rq, K)
        assert (ids == ID_NONE).all() and np.isnan(sc).all()


def test_first_delete_of_a_handle_is_a_delete_where(va, world):
    """No tombstone exists yet: the device bitmap is made by this call, as by the first vrod_index_delete."""
    _, queries, *_ = world
    ix, model = filled(va, world)
    with ix:
        same_searches(ix, model, queries[DIM], "before", paths=(PATH_AUTO,))
        p = GRID[21]
        assert ix.delete_where(p, allowed_only=True) == model.delete_where(p, ALLOWED) > 0
        same_state(ix, model, "first delete")
        same_searches(ix, model, queries[DIM], "after the first delete")


def test_delete_where_frees_keys(va, world):
    ix, model = filled(va, world)
    with ix:
        keys = np.arange(N, dtype=np.uint64) * np.uint64(3) + np.uint64(1000)
        keys[::5] = ID_NONE                                                      # rows without a key
        ix.set_keys(0, keys)
        before = ix.key_stats()["keyed_live"]
        assert before == int((keys != ID_NONE).sum())
        p = GRID[16]
        rows = model.matching(p, 0)
        keyed = rows[keys[rows] != ID_NONE]
        assert 0 < keyed.size < rows.size
        assert ix.delete_where(p) == model.delete_where(p, 0) == rows.size
        assert ix.key_stats()["keyed_live"] == before - keyed.size
        assert (ix.find_keys(keys[keyed]) == ID_NONE).all()                      # a dead row's key is not found ...
        live = np.flatnonzero(~model.deleted)
        assert np.array_equal(ix.find_keys(keys[live[keys[live] != ID_NONE]]), live[keys[live] != ID_NONE].astype(np.uint64))
        free = live[keys[live] == ID_NONE][:1]
        ix.set_keys(int(free[0]), keys[keyed[:1]])                               # ... and can be given to another row
        assert ix.find_keys(keys[keyed[:1]])[0] == free[0] and ix.key_stats()["keyed_live"] == before - keyed.size + 1


# ---------------------------------------------------------------- set_filter_where
def test_set_filter_where(va, world):
    corpora, queries, *_ = world
    rq = queries[DIM]
    ix, model = filled(va, world, restrict=True, off=OFF)
    rng = np.random.default_rng(77)
    with ix:
        same_searches(ix, model, rq, "before")
        old = model.allow.copy()
        p = (0, 0, 0, -3, I64_MAX, 0, 0)
        ix.set_filter_where(p, narrow=True)                                      # the intersection with the filter that is set
        model.set_filter_where(p, ALLOWED)
        assert np.array_equal(model.allow, old & model.hits(p)) and 0 < model.filter_count() < int((~model.deleted & model.hits(p)).sum())
        same_state(ix, model, "narrowed")
        same_searches(ix, model, rq, "narrowed")
        ix.set_filter_where(p)                                                   # replaces it
        model.set_filter_where(p, 0)
        same_state(ix, model, "replaced")
        same_searches(ix, model, rq, "replaced")
        # the where-clause of the forms that take no predicate
        thr = np.float32(0.3)
        (gl, gi, gs), (wl, wi, ws) = ix.range_search(rq, thr), model.range_search(rq, np.full(len(rq), thr, np.float32))
        assert 0 < int(wl[-1]) < len(rq) * model.filter_count() and np.array_equal(gl, wl) and np.array_equal(gi, wi)
        assert np.array_equal(bits(gs), bits(ws))
        gi, gs, gl = ix.search_grouped(rq, 3)
        wi, ws, wl = model.search_grouped(rq, 3)
        assert_same(gi, gs, wi, ws, "grouped")
        assert np.array_equal(gl, wl)
        by = (np.flatnonzero(~model.deleted)[:6] + OFF).astype(np.uint64)
        assert_same(*ix.search_by_ids(by, K), *model.search_by_ids(by, K), "by id")
        # rows added afterwards are not allowed
        more = rng.standard_normal((40, DIM)).astype(np.float32)
        ix.add(more)
        model.add(more)
        ix.set_values(OFF + N, np.full(40, 2, np.int64))
        model.set_values(OFF + N, np.full(40, 2, np.int64))
        same_state(ix, model, "rows added later")
        same_searches(ix, model, rq, "rows added later")
        assert ix.filter_count() == model.filter_count() < ix.count_where([p])[0]
        # two filters, a gather search after each: every one sees its own rows
        ix.set_path(PATH_GATHER)
        for q in (GRID[16], GRID[15], GRID[7], GRID[16]):
            ix.set_filter_where(q)
            model.set_filter_where(q, 0)
            assert ix.filter_count() == model.filter_count() > 0
            assert_same(*ix.search(rq, K), *model.search(rq, K), f"gather after {q}")
        ix.set_path(PATH_AUTO)
        ix.set_filter_where(GRID[24])                                            # unsatisfiable: a filter that allows nothing
        model.set_filter_where(GRID[24], 0)
        assert ix.filter_count() == 0 and ix.live_count() == model.live_count()
        ids, sc = ix.search(rq, K)
        assert (ids == ID_NONE).all() and np.isnan(sc).all()
        assert ix.count_where([MATCH_ALL], True)[0] == 0 and ix.count_where([MATCH_ALL])[0] == model.live_count()
        ix.set_filter_where(p, narrow=True)                                      # narrowing nothing stays nothing
        assert ix.filter_count() == 0
        ix.set_filter(None)                                                      # (NULL, 0) still clears
        model.set_filter(None)
        same_state(ix, model, "cleared")
        ix.set_filter_where(p, narrow=True)                                      # no filter set: the flag changes nothing
        model.set_filter_where(p, ALLOWED)
        same_state(ix, model, "narrow without a filter")
        same_searches(ix, model, rq, "narrow without a filter")


def test_snapshots_are_those_of_the_id_based_calls(va, world, tmp_path):
    """set_filter_where(p) on a handle with deleted rows == set_filter(the model's bits: a deleted row's bit = does it
    match); delete_where(p) == delete(ids): the files are byte-identical."""
    p = (1, 0, 0, -3, I64_MAX, 0, 0)
    a, model = filled(va, world, restrict=True, off=OFF)
    b, _ = filled(va, world, restrict=True, off=OFF)
    with a, b:
        bits = model.filter_bits(p, 0)
        assert (bits & model.deleted).any() and (~bits & model.deleted).any()
        a.set_filter_where(p)
        b.set_filter(bits)
        fa, fb = str(tmp_path / "a.vrod"), str(tmp_path / "b.vrod")
        a.save(fa)
        b.save(fb)
        assert open(fa, "rb").read() == open(fb, "rb").read()
        model.set_filter(bits)
        q = GRID[16]
        ids = model.select_where(q, 0)
        assert ids.size and a.delete_where(q) == ids.size
        b.delete(ids)
        a.save(fa)
        b.save(fb)
        assert open(fa, "rb").read() == open(fb, "rb").read()
        assert va.snapshot_info(fa)["live_count"] == model.live_count() - ids.size


# ---------------------------------------------------------------- set_tags_where
def test_set_tags_where(va, world):
    _, queries, *_ = world
    rq = queries[DIM]
    ix, model = filled(va, world, restrict=True, off=OFF)
    with ix:
        def both(p, set_bits, clear_bits, flags, what):
            before = model.tags.copy()
            got = ix.set_tags_where(p, set_bits, clear_bits, allowed_only=bool(flags))
            want = model.set_tags_where(p, set_bits, clear_bits, flags)
            assert got == want, what
            assert np.array_equal(ix.get_tags(OFF, N), model.tags), what
            assert np.array_equal(model.tags[model.deleted], before[model.deleted]), what   # deleted rows keep their old mask
            return got
        assert both((0, 0, 0, *FULL, 1, 1), 1 << 40, 0, 0, "grant a group to tenant 1") > 0
        assert both((0, 0, 0, *FULL, 1, 1), 1 << 40, 0, 0, "again") == 0
        assert both((1 << 40, 0, 0, I64_MIN, -1, 0, 0), 0, (1 << 40) | B63, ALLOWED, "revoke it, and bit 63, where the filter allows") > 0
        assert both(MATCH_ALL, B63, 7, 0, "every live row") > 0
        assert both(MATCH_ALL, 0, 0, 0, "nothing to do") == 0
        assert both(GRID[24], 1, 0, 0, "unsatisfiable") == 0
        preds = [(B63, 0, 0), (1 << 40, 0, 0), (0, B63, 7), (0, 0, B63)] * 3
        assert_same(*ix.search_tagged(rq, K, np.array(preds, np.uint64)), *model.search_tagged(rq, K, preds), "search_tagged after")
        rc = ix._L.vrod_index_set_tags_where(ix._h, ix._row_preds(MATCH_ALL, 1).ctypes.data, 0, 3, 1, None)   # set_bits & clear_bits != 0
        assert rc == ERR_INVALID_ARG and np.array_equal(ix.get_tags(OFF, N), model.tags)


def test_set_tags_where_on_a_handle_without_tags(va, world, tmp_path):
    ix, model = filled(va, world, tags=False, restrict=True)
    f = str(tmp_path / "t.vrod")
    with ix:
        assert ix.set_tags_where(MATCH_ALL, 0, 0xFF) == 0 and ix.set_tags_where(GRID[16], 0, 0) == 0
        ix.save(f)
        assert va.snapshot_info(f)["has_tags"] == 0                              # nothing was allocated
        p = GRID[16]
        assert ix.set_tags_where(p, B63 | 2, 1) == model.set_tags_where(p, B63 | 2, 1, 0) == model.matching(p, 0).size > 0
        assert np.array_equal(ix.get_tags(0, N), model.tags)
        ix.save(f)
        assert va.snapshot_info(f)["has_tags"] == 1                              # the column is created by this call
        with va.Index.load(f) as loaded:
            assert np.array_equal(loaded.get_tags(0, N), model.tags)
        assert ix.count_where([(B63, 2, 1, *FULL, 7, 1)])[0] == model.count_where([(B63, 2, 1, *FULL, 7, 1)])[0] > 0


# ---------------------------------------------------------------- refusals
def test_a_pending_search_blocks_every_operation(va, world):
    import torch
    ix, model = filled(va, world, restrict=True)
    with ix:
        oi = torch.empty((4, K), dtype=torch.int64, device="cuda")
        osc = torch.empty((4, K), dtype=torch.float32, device="cuda")
        ix.search_begin_synthetic_device(2, 0, 4, K, oi, osc)
        p = GRID[7]
        for call in (lambda: ix.count_where([p]), lambda: ix.select_where(p), lambda: ix.select_where_device(p, 10), lambda: ix.delete_where(p),
                     lambda: ix.set_filter_where(p), lambda: ix.set_tags_where(p, 1 << 50, 0)):
            with pytest.raises(va.VrodError) as e:
                call()
            assert e.value.code == ERR_INVALID_ARG
        ix.search_end()
        same_state(ix, model, "after the refused calls")
        assert np.array_equal(ix.get_tags(0, N), model.tags)
        assert ix.delete_where(p) == model.delete_where(p, 0) > 0                # after search_end they work


def test_a_multi_device_handle_is_unsupported(va, world):
    corpora = world[0]
    with va.Index(DIM, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(corpora[DIM])
        L, pp = ix._L, ix._row_preds(MATCH_ALL, 1)
        out = np.full(4, 7, np.uint64)
        n = C.c_uint64(7)
        assert L.vrod_index_count_where(ix._h, pp.ctypes.data, 1, 0, out.ctypes.data) == ERR_UNSUPPORTED
        assert L.vrod_index_select_where(ix._h, pp.ctypes.data, 0, 4, C.byref(n), out.ctypes.data) == ERR_UNSUPPORTED
        assert L.vrod_index_select_where_device(ix._h, pp.ctypes.data, 0, 0, C.byref(n), None, None) == ERR_UNSUPPORTED
        assert L.vrod_index_delete_where(ix._h, pp.ctypes.data, 0, C.byref(n)) == ERR_UNSUPPORTED
        assert L.vrod_index_set_filter_where(ix._h, pp.ctypes.data, 0) == ERR_UNSUPPORTED
        assert L.vrod_index_set_tags_where(ix._h, pp.ctypes.data, 0, 1, 0, C.byref(n)) == ERR_UNSUPPORTED
        assert (out == 7).all() and n.value == 7                                 # outputs untouched
        assert (ix.count, ix.live_count(), ix.filter_count()) == (N, N, N) and not ix.get_tags(0, 50).any()
