"""GPU tests of the candidate-list searches (vrod_search_candidates, vrod_score_candidates) against
tests/candidates_model.py.

The contract: query q sees the distinct ids of its own list that are current, live, allowed rows; the search form returns
what vrod_search returns on a handle holding only those rows (ids mapped back), the score form the canonical score of every
listed id at its own position and NaN where the id is ignored.  Expected values come from the model (np.unique, the
eligible rows, support.oracle_over); ids and score bits are compared with support.assert_same.

Shapes: 4000 rows (the 16384-entry lists therefore repeat ids and name stale ones), d = 1, 33 and 768, batches of 1, 9 and
70 queries; list lengths 0, 1, 2, 63, 64, 65 (both sides of the 64-entry tile of the score launch and of a wave of the
sort), 1000 and 16384 (the three work-group classes of the sort: networks of 256, 4096 and 16384 entries).
"""
import ctypes as C

import numpy as np
import pytest

import candidates_model as M
import support
from support import ID_NONE, PATH_GATHER, va, O, bits, eligible_rows, row_bytes  # noqa: F401

pytestmark = pytest.mark.gpu

N, K = 4000, 10
LENGTHS = [0, 1, 2, 63, 64, 65, 1000, 16384]
SENT_ID, SENT_SC = np.uint64(0x5A5A5A5A5A5A5A5A), np.float32(-12345.5)
SENT32 = 0x5A5A5A5A


def raw_corpus(n, d, metric, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    if metric == "ip":   # norms spread over e^2
        raw *= np.exp(rng.uniform(-1.0, 1.0, (n, 1))).astype(np.float32)
    return raw


_CACHE = {}


def corpus(d, metric, n=N):
    """The raw rows of one (shape, metric): computed once, shared, never written to."""
    key = (n, d, metric)
    if key not in _CACHE:
        raw = raw_corpus(n, d, metric, 7000 + d)
        raw.setflags(write=False)
        _CACHE[key] = raw
    return _CACHE[key]


def make_index(va, raw, dtype, metric, id_offset=0):
    ix = va.Index(raw.shape[1], dtype, metric)
    ix.add(raw)
    if id_offset:
        ix.set_id_offset(id_offset)
    return ix


def make_lists(rng, lengths, n, id_offset=0, stale=40):
    """One list per length: ids drawn from [0, n + stale) -- the last `stale` of them are past the count -- distinct while the
    length allows it, given in random, ascending or descending order by the query's position."""
    lists = []
    for q, L in enumerate(lengths):
        hi = n + stale
        ids = rng.choice(hi, L, replace=False) if L <= hi else rng.integers(0, hi, L)
        if q % 3 == 1:
            ids = np.sort(ids)
        elif q % 3 == 2:
            ids = np.sort(ids)[::-1]
        lists.append((ids.astype(np.uint64) + np.uint64(id_offset)))
    return lists


def lengths_for(nq):
    if nq == 1:
        return [1000]
    return [(LENGTHS + [300])[q % 9] for q in range(nq)]


def both(ix, rq, k, lists):
    ids, lims = M.flat(lists)
    return ix.search_candidates(rq, k, ids, cand_lims=lims), ix.score_candidates(rq, ids, cand_lims=lims)


def check_both(O, ix, raw, rq, k, dtype, metric, lists, eligible, id_offset=0, what=""):
    (gi, gs), sc = both(ix, rq, k, lists)
    wi, ws = M.search(O, raw, rq, k, dtype, metric, lists, eligible, id_offset)
    support.assert_same(gi, gs, wi, ws, f"{what}: search form")
    support.assert_scores_same(sc, M.score(O, raw, rq, dtype, metric, lists, eligible, id_offset), f"{what}: score form")
    return (gi, gs), sc


def p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw_search(ix, rq, k, ids, lims, nq=None):
    """The host search form through ctypes, outputs preset to sentinels -> (rc, ids, scores)."""
    nq = rq.shape[0] if nq is None else nq
    oi = np.full((nq, max(k, 1)), SENT_ID, np.uint64)
    sc = np.full((nq, max(k, 1)), SENT_SC, np.float32)
    rc = ix._L.vrod_search_candidates(ix._h, p(rq), nq, k, p(lims), p(ids), p(oi), p(sc))
    return rc, oi, sc


def raw_score(ix, rq, ids, lims, nq=None):
    nq = rq.shape[0] if nq is None else nq
    sc = np.full(max(int(ids.size), 1), SENT_SC, np.float32)
    rc = ix._L.vrod_score_candidates(ix._h, p(rq), nq, p(lims), p(ids), p(sc))
    return rc, sc


def untouched(*arrays):
    return all((a == (SENT_ID if a.dtype == np.uint64 else SENT_SC)).all() for a in arrays)


def device_both(va, ix, rq, k, lists, expect_code=None):
    """Both device forms, every input made on a side stream just before the call -> ((ids, scores), flat scores) as numpy;
    after refused calls (expect_code) the outputs as they are."""
    import torch
    dev = torch.device("cuda:0")
    ids, lims = M.flat(lists)
    nq = rq.shape[0]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        dq = torch.from_numpy(np.array(rq, dtype=np.float32)).to(dev, non_blocking=True)
        d_lims = torch.from_numpy(lims.view(np.int32).copy()).to(dev, non_blocking=True)
        d_ids = torch.from_numpy(ids.view(np.int64).copy()).to(dev, non_blocking=True)
        oi = torch.full((nq, k), SENT32, dtype=torch.int64, device=dev)
        osc = torch.full((nq, k), float(SENT_SC), dtype=torch.float32, device=dev)
        fsc = torch.full((max(int(ids.size), 1),), float(SENT_SC), dtype=torch.float32, device=dev)
        if expect_code is None:
            ix.search_candidates_device(dq, k, d_lims, d_ids, out_ids=oi, out_scores=osc)
            ix.score_candidates_device(dq, d_lims, d_ids, out_scores=fsc)
        else:
            for call in (lambda: ix.search_candidates_device(dq, k, d_lims, d_ids, out_ids=oi, out_scores=osc),
                         lambda: ix.score_candidates_device(dq, d_lims, d_ids, out_scores=fsc)):
                with pytest.raises(va.VrodError) as e:
                    call()
                assert e.value.code == expect_code
    return (oi.cpu().numpy().view(np.uint64), osc.cpu().numpy()), fsc.cpu().numpy()[:ids.size if expect_code is None else None]


# ------------------------------------------------------------------ 1. parity of both forms with the model
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [1, 33, 768])
@pytest.mark.parametrize("nq", [1, 9, 70])
def test_both_forms_match_the_model(va, O, nq, d, dtype, metric):
    raw = corpus(d, metric)
    rng = np.random.default_rng(100 * nq + d)
    rq = rng.standard_normal((nq, d)).astype(np.float32)
    lists = make_lists(rng, lengths_for(nq), N)
    with make_index(va, raw, dtype, metric) as ix:
        check_both(O, ix, raw, rq, K, dtype, metric, lists, np.arange(N), what=f"nq {nq} d {d} {dtype} {metric}")


# ------------------------------------------------------------------ 2. repeats
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_repeated_ids_count_once(va, O, dtype):
    raw = corpus(33, "cosine")
    rng = np.random.default_rng(2)
    rq = rng.standard_normal((3, 33)).astype(np.float32)
    twice = rng.permutation(np.concatenate([np.arange(500, 1500), np.arange(500, 1500)]))
    lists = [np.full(16384, 77, np.uint64), twice.astype(np.uint64), np.array([5, 5, 5], np.uint64)]
    with make_index(va, raw, dtype, "cosine") as ix:
        (gi, gs), sc = check_both(O, ix, raw, rq, K, dtype, "cosine", lists, np.arange(N), what="repeats")
    # one id 16384 times: one result, and its score at every position
    assert gi[0, 0] == 77 and (gi[0, 1:] == ID_NONE).all() and np.isnan(gs[0, 1:]).all()
    assert (bits(sc[:16384]) == bits(gs[0, :1])).all()
    # every id twice: each row once in the result, the same bits at both positions
    assert len(set(gi[1].tolist())) == K and ID_NONE not in gi[1]
    s2 = sc[16384:16384 + 2000]
    order = np.argsort(twice, kind="stable")
    assert np.array_equal(bits(s2[order[0::2]]), bits(s2[order[1::2]]))
    assert gi[2, 0] == 5 and (gi[2, 1:] == ID_NONE).all()


# ------------------------------------------------------------------ 3. stale, deleted and disallowed ids
@pytest.mark.parametrize("dtype,metric", [("f32", "l2"), ("bf16", "ip")])
def test_ignored_ids(va, O, dtype, metric):
    raw = corpus(33, metric)
    off = 1000
    rng = np.random.default_rng(3)
    rq = rng.standard_normal((3, 33)).astype(np.float32)
    deleted = [10, 11, 2000]
    allow = np.ones(N, bool)
    allow[[20, 21, 3000]] = False
    el = eligible_rows(N, allow=allow, deleted=deleted)
    # local rows 5, 30, 31 are fine; below the offset, past the count, ID_NONE, deleted, disallowed are not
    l0 = np.array([off + 5, off - 1, 0, off + N, off + N + 7, int(ID_NONE), off + 10, off + 2000, off + 20, off + 3000, off + 30, off + 31,
                   1 << 40], np.uint64)
    l1 = np.array([off - 1, 999, off + N, int(ID_NONE), off + 11, off + 21], np.uint64)        # nothing eligible in it
    l2 = np.arange(off - 50, off + N + 50, dtype=np.uint64)[::-1].copy()                      # every id and a margin, descending
    lists = [l0, l1, l2]
    with make_index(va, raw, dtype, metric, id_offset=off) as ix:
        ix.delete(np.array(deleted, np.uint64) + np.uint64(off))
        ix.set_filter(allow)
        (gi, gs), sc = check_both(O, ix, raw, rq, K, dtype, metric, lists, el, id_offset=off, what="ignored ids")
    assert sorted(gi[0, :3].tolist()) == [off + 5, off + 30, off + 31] and (gi[0, 3:] == ID_NONE).all()
    assert np.isnan(sc[:l0.size]).tolist() == [False, True, True, True, True, True, True, True, True, True, False, False, True]
    assert (gi[1] == ID_NONE).all() and np.isnan(gs[1]).all() and np.isnan(sc[l0.size:l0.size + l1.size]).all()
    rows2 = l2.astype(np.int64) - off
    want_nan = ~np.isin(rows2, el)
    assert np.array_equal(np.isnan(sc[l0.size + l1.size:]), want_nan)


# ------------------------------------------------------------------ 4. ties
def test_duplicate_rows_rank_by_id_whatever_the_list_order(va, O):
    raw = corpus(33, "cosine").copy()
    raw[3100] = raw[40]
    raw[900] = raw[40]
    rq = np.ascontiguousarray(raw[40][None, :])                                                # the duplicates are its best match
    lists = [np.array([3100, 900, 40, 7, 8], np.uint64)]                                       # larger ids first
    with make_index(va, raw, "f32", "cosine") as ix:
        (gi, gs), sc = check_both(O, ix, raw, rq, 4, "f32", "cosine", lists, np.arange(N), what="ties")
    assert gi[0, :3].tolist() == [40, 900, 3100] and len(set(bits(gs[0, :3]).tolist())) == 1
    assert len(set(bits(sc[:3]).tolist())) == 1


# ------------------------------------------------------------------ 5. k
def test_k_beyond_the_set_and_at_its_maximum(va, O):
    raw = corpus(33, "l2")
    rng = np.random.default_rng(5)
    rq = rng.standard_normal((2, 33)).astype(np.float32)
    lists = make_lists(rng, [16384, 7], N)
    with make_index(va, raw, "bf16", "l2") as ix:
        ids, lims = M.flat(lists)
        gi, gs = ix.search_candidates(rq, va.MAX_K, ids, cand_lims=lims)
        wi, ws = M.search(O, raw, rq, va.MAX_K, "bf16", "l2", lists, np.arange(N))
        support.assert_same(gi, gs, wi, ws, "k = MAX_K")
        assert ID_NONE not in gi[0]                                                            # 16384 draws of 4040 ids: far more than 3584 rows
        n1 = M.candidate_rows(lists[1], N, np.arange(N)).size
        assert (gi[1, :n1] != ID_NONE).all() and (gi[1, n1:] == ID_NONE).all() and np.isnan(gs[1, n1:]).all()


# ------------------------------------------------------------------ 6. the life of a handle
def test_after_update_delete_compact_labels_and_tags(va, O):
    raw = corpus(33, "cosine").copy()
    rng = np.random.default_rng(6)
    rq = rng.standard_normal((4, 33)).astype(np.float32)
    lists = make_lists(rng, [300, 65, 1000, 2], N)
    with make_index(va, raw, "bf16", "cosine") as ix:
        before = check_both(O, ix, raw, rq, K, "bf16", "cosine", lists, np.arange(N), what="fresh")
        # labels and tags do not matter
        ix.set_labels(0, rng.integers(0, 5, N).astype(np.uint32))
        ix.set_tags(0, rng.integers(0, 1 << 20, N).astype(np.uint64))
        (gi, gs), sc = both(ix, rq, K, lists)
        support.assert_same(gi, gs, *before[0], "labels and tags set")
        support.assert_scores_same(sc, before[1], "labels and tags set")
        # an updated candidate row is scored as it is now
        row = int(next(x for x in lists[0] if x < N))
        raw[row] = rq[0] * np.float32(3.0)
        ix.update([row], raw[row][None, :])
        (gi, gs), sc = check_both(O, ix, raw, rq, K, "bf16", "cosine", lists, np.arange(N), what="after update")
        assert gi[0, 0] == row
        # delete + compact: the rows move down, ids past the new count are stale
        gone = np.sort(rng.choice(N, 600, replace=False))
        ix.delete(gone)
        check_both(O, ix, raw, rq, K, "bf16", "cosine", lists, eligible_rows(N, deleted=gone), what="after delete")
        ix.compact()
        kept = np.delete(raw, gone, axis=0)
        assert ix.count == N - 600
        check_both(O, ix, kept, rq, K, "bf16", "cosine", lists, np.arange(N - 600), what="after compact")


# ------------------------------------------------------------------ 7. refusals leave the outputs untouched
def test_refusals_on_a_live_handle(va, O):
    raw = corpus(33, "cosine")
    rq = np.ascontiguousarray(raw[:2])
    ids = np.arange(10, dtype=np.uint64)
    ok = np.array([0, 4, 10], np.uint32)
    with make_index(va, raw, "f32", "cosine") as ix:
        def refused(lims, k=K, q=rq, cand=ids, code=1, what=""):
            rc, oi, sc = raw_search(ix, q, k, cand, lims)
            assert rc == code and untouched(oi, sc), f"search form: {what}"
            if k == K:
                rc, sc = raw_score(ix, q, cand, lims)
                assert rc == code and untouched(sc), f"score form: {what}"

        refused(np.array([1, 4, 10], np.uint32), what="lims[0] != 0")
        refused(np.array([0, 6, 5], np.uint32), what="lims decreases")
        long_ids = np.zeros(16385 + 3, np.uint64)
        refused(np.array([0, 3, 16388], np.uint32), cand=long_ids, what="a 16385-entry list")
        rc, oi, sc = raw_search(ix, rq, K, long_ids, np.array([0, 4, 16388], np.uint32))         # 16384 entries pass
        assert rc == 0 and oi[1, 0] == 0
        refused(ok, k=0, what="k = 0")
        refused(ok, k=va.MAX_K + 1, what="k > MAX_K")
        bad = rq.copy()
        bad[1, 5] = np.nan
        refused(ok, q=bad, code=2, what="NaN query")
        bad[1, 5] = np.inf
        refused(ok, q=bad, code=2, what="Inf query")
        # null required pointers
        oi = np.full((2, K), SENT_ID, np.uint64)
        sc = np.full((2, K), SENT_SC, np.float32)
        L, h = ix._L, ix._h
        for a in ((None, p(ok), p(ids), p(oi), p(sc)), (p(rq), None, p(ids), p(oi), p(sc)), (p(rq), p(ok), None, p(oi), p(sc)),
                  (p(rq), p(ok), p(ids), None, p(sc)), (p(rq), p(ok), p(ids), p(oi), None)):
            assert L.vrod_search_candidates(h, a[0], 2, K, a[1], a[2], a[3], a[4]) == 1
            assert untouched(oi, sc)
        for a in ((None, p(ok), p(ids), p(sc)), (p(rq), None, p(ids), p(sc)), (p(rq), p(ok), None, p(sc)), (p(rq), p(ok), p(ids), None)):
            assert L.vrod_score_candidates(h, a[0], 2, a[1], a[2], a[3]) == 1
            assert untouched(sc)
        # nq == 0 is fine and writes nothing
        assert L.vrod_search_candidates(h, None, 0, K, None, None, None, None) == 0
        assert L.vrod_score_candidates(h, None, 0, None, None, None) == 0
        # the handle is as usable as before
        check_both(O, ix, raw, rq, K, "f32", "cosine", [ids[:4], ids[4:]], np.arange(N), what="after the refusals")


def test_pending_search_blocks_every_form(va, O):
    import torch
    raw = corpus(33, "cosine")
    dev = torch.device("cuda:0")
    rq = np.ascontiguousarray(raw[:2])
    lists = [np.arange(4, dtype=np.uint64), np.arange(4, 10, dtype=np.uint64)]
    ids, lims = M.flat(lists)
    with make_index(va, raw, "bf16", "cosine") as ix:
        dq = torch.from_numpy(raw[:4].copy()).to(dev)
        oi = torch.empty((4, K), dtype=torch.int64, device=dev)
        osc = torch.empty((4, K), dtype=torch.float32, device=dev)
        ix.search_begin_device(dq, K, oi, osc)
        assert ix.pending == 1
        rc, hi, hs = raw_search(ix, rq, K, ids, lims)
        assert rc == 1 and untouched(hi, hs)
        rc, hs = raw_score(ix, rq, ids, lims)
        assert rc == 1 and untouched(hs)
        (di, ds), fs = device_both(va, ix, rq, K, lists, expect_code=1)
        assert (di == SENT32).all() and (ds == SENT_SC).all() and (fs == SENT_SC).all()
        assert ix.pending == 1
        ix.search_end()
        check_both(O, ix, raw, rq, K, "bf16", "cosine", lists, np.arange(N), what="after the pending search")


def test_multi_device_handle_is_unsupported(va, O):
    raw = corpus(33, "cosine")
    rq = np.ascontiguousarray(raw[:2])
    lists = [np.arange(4, dtype=np.uint64), np.arange(4, 10, dtype=np.uint64)]
    ids, lims = M.flat(lists)
    with va.Index(33, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        rc, hi, hs = raw_search(ix, rq, K, ids, lims)
        assert rc == 6 and untouched(hi, hs)
        rc, hs = raw_score(ix, rq, ids, lims)
        assert rc == 6 and untouched(hs)
        (di, ds), fs = device_both(va, ix, rq, K, lists, expect_code=6)
        assert (di == SENT32).all() and (ds == SENT_SC).all() and (fs == SENT_SC).all()


def test_empty_handle_and_no_eligible_row(va, O):
    raw = corpus(33, "cosine")
    rq = np.ascontiguousarray(raw[:2]).copy()
    rq[0, 0] = np.nan                                                                          # the queries are not looked at
    lists = [np.arange(4, dtype=np.uint64), np.arange(4, 10, dtype=np.uint64)]
    with va.Index(33, "bf16", "cosine") as ix:
        (gi, gs), sc = both(ix, rq, K, lists)
        assert (gi == ID_NONE).all() and np.isnan(gs).all() and sc.size == 10 and np.isnan(sc).all()
    with make_index(va, raw, "bf16", "cosine") as ix:
        ix.set_filter(np.zeros(N, bool))
        (gi, gs), sc = both(ix, rq, K, lists)
        assert (gi == ID_NONE).all() and np.isnan(gs).all() and sc.size == 10 and np.isnan(sc).all()
        ix.set_filter(None)
        rq[0, 0] = 1.0
        (gi, gs), sc = both(ix, rq, K, [[], []])                                               # every list empty
        assert (gi == ID_NONE).all() and np.isnan(gs).all() and sc.size == 0


# ------------------------------------------------------------------ 8. the device forms
@pytest.mark.parametrize("dtype,metric", [("f32", "ip"), ("bf16", "l2")])
def test_device_forms_match_the_host_forms(va, O, dtype, metric):
    raw = corpus(33, metric)
    rng = np.random.default_rng(8)
    lengths = [65, 0, 16384, 1, 1000, 64, 300, 2, 63, 5, 130]
    rq = rng.standard_normal((len(lengths), 33)).astype(np.float32)
    off = 1 << 33
    lists = make_lists(rng, lengths, N, id_offset=off)
    with make_index(va, raw, dtype, metric, id_offset=off) as ix:
        ix.delete(np.arange(100, 300, dtype=np.uint64) + np.uint64(off))
        (hi, hs), hsc = both(ix, rq, K, lists)
        (di, ds), dsc = device_both(va, ix, rq, K, lists)
        assert np.array_equal(hi, di) and np.array_equal(bits(hs), bits(ds)) and np.array_equal(bits(hsc), bits(dsc))
        wi, ws = M.search(O, raw, rq, K, dtype, metric, lists, eligible_rows(N, deleted=np.arange(100, 300)), off)
        support.assert_same(hi, hs, wi, ws, "the host form itself")


# ------------------------------------------------------------------ 9. stats
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stats(va, O, dtype):
    d = 33
    raw = corpus(d, "cosine")
    rq = np.ascontiguousarray(raw[:4])
    # resolved sets: 90 rows (100 listed, 10 deleted), 3 rows listed 3 times each, none, 1 row
    lists = [np.arange(100, 200, dtype=np.uint64), np.array([7, 8, 9] * 3, np.uint64), np.array([N, N + 1, int(ID_NONE)], np.uint64),
             np.array([3999], np.uint64)]
    ids, lims = M.flat(lists)
    with make_index(va, raw, dtype, "cosine") as ix:
        ix.delete(np.arange(150, 160, dtype=np.uint64))
        ix.set_path(va.PATH_EXACT)                                                             # ignored
        ix.search_candidates(rq, K, ids, cand_lims=lims)
        st = ix.last_stats()
        rows = 90 + 3 + 0 + 1
        assert (st["path"], st["nq"], st["k"], st["kprime"]) == (PATH_GATHER, 4, K, 90), st
        assert st["scan_launches"] == 1 and st["fallback_queries"] == 0 and st["band_queries"] == 0, st
        assert st["max_fast_err"] == 0 and st["eps_bound"] == 0, st
        assert st["scan_bytes"] == rows * row_bytes(dtype, d) and st["scan_flops"] == 2.0 * rows * d, st
        ix.score_candidates(rq, ids, cand_lims=lims)
        st = ix.last_stats()
        rows = 90 + 9 + 0 + 1                                                                  # every eligible entry is scored, repeats included
        assert (st["path"], st["nq"], st["k"], st["kprime"]) == (PATH_GATHER, 4, 0, 90), st
        assert st["scan_launches"] == 1 and st["fallback_queries"] == 0 and st["band_queries"] == 0, st
        assert st["scan_bytes"] == rows * row_bytes(dtype, d) and st["scan_flops"] == 2.0 * rows * d, st
