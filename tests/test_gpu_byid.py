"""GPU tests of the searches whose queries are stored rows (vrod_search_by_ids, vrod_knn_graph) against the CPU oracle.

The contract: query q is the PREPARED stored row ids[q], used as stored -- not normalised again, not rounded again -- and
its result row is the oracle's canonical scan of that prepared row over the eligible rows (live, allowed), bit for bit.
Expected values therefore come from oracle.prepare (the corpus, once) + oracle.scan_topk with the prepared rows themselves
as queries -- the oracle's form that takes prepared inputs -- over the eligible rows only, ids mapped back.  The self drop
is restated in numpy: the (k + 1)-list minus the entry that carries the query's own id, cut to k.

Shapes: 3000 rows, d = 72 (a row stride with padding) and 128, every dtype and metric; the inner-product corpus has its
rows scaled by exp(U(-1, 1)) so that a row is often not its own best match.  The graph runs over 2 * batch + 300 rows:
three batches, both workspaces reused, a partial tail.
"""
import ctypes as C

import numpy as np
import pytest

import support
from support import (  # noqa: F401
    DT, METRIC_COSINE, METRIC_L2, PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, THREADS, va, O, bits, drop_self)

pytestmark = pytest.mark.gpu

N, K = 3000, 10
SENT_ID, SENT_SC = np.uint64(0x5A5A5A5A5A5A5A5A), np.float32(-12345.5)


def assert_same(got, want, what=""):
    support.assert_same(*got, *want, what)


def raw_corpus(n, d, metric, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    if metric == "ip":   # norms spread over e^2: a row is often not its own best match
        raw *= np.exp(rng.uniform(-1.0, 1.0, (n, 1))).astype(np.float32)
    return raw


def prepare(O, raw, dtype, metric):
    return O.prepare(raw, DT[dtype], METRIC_COSINE if metric == "cosine" else METRIC_L2, threads=THREADS)


_CACHE = {}


def corpus(O, d, dtype, metric, n=N):
    """(raw rows, prepared rows) of one (shape, dtype, metric): computed once, shared, never written to."""
    key = (n, d, dtype, metric)
    if key not in _CACHE:
        raw = raw_corpus(n, d, metric, 1000 + d)
        pc = prepare(O, raw, dtype, metric)
        raw.setflags(write=False)
        pc.setflags(write=False)
        _CACHE[key] = (raw, pc)
    return _CACHE[key]


def expect(O, pc, metric, qrows, k, elig=None, exclude_self=False, id_offset=0):
    """pc: the prepared corpus; qrows: the queries' local rows; elig: None or a bool mask of the rows a search may return."""
    scan = METRIC_L2 if metric == "l2" else METRIC_COSINE
    qrows = np.asarray(qrows, np.int64)
    rows = np.arange(pc.shape[0]) if elig is None else np.flatnonzero(elig)
    k1 = k + 1 if exclude_self else k
    i, s = O.scan_topk(np.ascontiguousarray(pc[rows]).reshape(rows.size, pc.shape[1]), np.ascontiguousarray(pc[qrows]), k1, scan,
                       threads=THREADS)
    none = i == ID_NONE
    at = np.where(none, 0, i).astype(np.int64)                 # positions in `rows` -> local rows -> ids
    ids = np.where(none, ID_NONE, (rows[at] if rows.size else at).astype(np.uint64) + np.uint64(id_offset))
    if not exclude_self:
        return ids, s
    return drop_self(ids, s, qrows.astype(np.uint64) + np.uint64(id_offset), k)


def make_index(va, raw, dtype, metric, id_offset=0):
    ix = va.Index(raw.shape[1], dtype, metric)
    ix.add(raw)
    if id_offset:
        ix.set_id_offset(id_offset)
    return ix


# ------------------------------------------------------------------ every route, dtype, metric and row stride
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [72, 128])
def test_routes_match_the_oracle(va, O, d, dtype, metric):
    raw, pc = corpus(O, d, dtype, metric)
    rng = np.random.default_rng(7)
    plans = [(PATH_AUTO, 1), (PATH_AUTO, 40), (PATH_AUTO, 300), (PATH_STREAM, 40), (PATH_MFMA, 40), (PATH_EXACT, 40), (PATH_GATHER, 40)]
    with make_index(va, raw, dtype, metric) as ix:
        for path, nq in plans:
            ix.set_path(path)
            q = rng.choice(N, nq, replace=False)
            for ex in (False, True):
                got = ix.search_by_ids(q, K, exclude_self=ex)
                st = ix.last_stats()
                assert_same(got, expect(O, pc, metric, q, K, exclude_self=ex), f"path {path} nq {nq} exclude {ex}")
                assert st["k"] == K and st["nq"] == nq
                if path != PATH_AUTO:
                    assert st["path"] == path, st
                if ex:
                    assert not (got[0] == q[:, None].astype(np.uint64)).any()
                elif metric == "l2":   # the stored row is the query bit for bit: its distance to itself is +0.0
                    hit = got[0] == q[:, None].astype(np.uint64)
                    assert hit.sum(axis=1).tolist() == [1] * nq
                    assert (bits(got[1])[hit] == 0).all()


def test_ip_rows_are_often_not_their_own_best_match(va, O):
    """The premise of the inner-product cases above, from the oracle: the drop cannot be 'skip position 0'."""
    _, pc = corpus(O, 72, "f32", "ip")
    q = np.arange(300)
    ids, _ = expect(O, pc, "ip", q, 1)
    assert (ids[:, 0] != q.astype(np.uint64)).sum() >= 30


# ------------------------------------------------------------------ "as stored"
def test_query_is_the_stored_row_not_a_second_preparation(va, O):
    """Cosine bf16: the stored row is a normalised vector rounded to bf16; preparing it AGAIN (what a read-back followed by
    vrod_search does) normalises the rounded vector and rounds once more.  The library must give the scores of the row as
    stored.

    At d = 72 and d = 128 the second preparation changes no stored row of this file's Gaussian corpora for any seed in
    0 .. 7 (checked with the oracle: the norm of a rounded unit vector is off by ~2^-9 / sqrt(d), too little to move a
    bf16 value across a rounding boundary), so those shapes cannot show the difference and the case runs at d = 8, where
    about one row in a hundred changes.  The premise is asserted from the oracle before the library is asked."""
    for big_d in (72, 128):
        for seed in range(8):
            pc = prepare(O, raw_corpus(N, big_d, "cosine", 5000 + seed), "bf16", "cosine")
            assert np.array_equal(bits(prepare(O, pc, "bf16", "cosine")), bits(pc)), (big_d, seed)
    d = 8
    for seed in range(8):
        raw = raw_corpus(N, d, "cosine", 5000 + seed)
        pc = prepare(O, raw, "bf16", "cosine")
        pc2 = prepare(O, pc, "bf16", "cosine")
        changed = np.flatnonzero((bits(pc2) != bits(pc)).any(axis=1))
        if changed.size == 0:
            continue
        q = np.concatenate([changed[:48], np.arange(16)])
        as_is = expect(O, pc, "cosine", q, K)
        again = O.scan_topk(pc, np.ascontiguousarray(pc2[q]), K, METRIC_COSINE, threads=THREADS)
        if not np.array_equal(bits(as_is[1]), bits(again[1])):
            break
    else:
        pytest.fail("no seed in 0..7 makes the second preparation visible: the case shows nothing")
    with make_index(va, raw, "bf16", "cosine") as ix:
        back = ix.get_rows(0, N)
        assert np.array_equal(bits(back), bits(pc))
        assert_same(ix.search(back[q], K), again, "read back + vrod_search prepares a second time")
        for ex in (False, True):
            assert_same(ix.search_by_ids(q, K, exclude_self=ex), expect(O, pc, "cosine", q, K, exclude_self=ex), f"as stored, exclude {ex}")


# ------------------------------------------------------------------ the self drop
@pytest.mark.parametrize("dtype,metric,d", [("bf16", "cosine", 72), ("f32", "l2", 128), ("f32", "ip", 72)])
def test_self_drop_is_by_id(va, O, dtype, metric, d):
    base, _ = corpus(O, d, dtype, metric)
    raw = base.copy()
    raw[256:512] = np.tile(raw[256:320], (4, 1))
    pc = prepare(O, raw, dtype, metric)
    dup = np.arange(256, 512)                       # 64 rows, four copies each: rows r, r + 64, r + 128, r + 192
    off = 10 ** 9
    with make_index(va, raw, dtype, metric, id_offset=off) as ix:
        # exact duplicates: self sits at position 0 .. 3 of its own list (ties break by the smaller id)
        full = expect(O, pc, metric, dup, K, id_offset=off)
        if metric != "ip":
            pos = np.argmax(full[0] == (dup[:, None] + off).astype(np.uint64), axis=1)
            assert set(pos.tolist()) == {0, 1, 2, 3}
        for path in (PATH_AUTO, PATH_MFMA):
            ix.set_path(path)
            assert_same(ix.search_by_ids(dup + off, K, exclude_self=True), expect(O, pc, metric, dup, K, exclude_self=True, id_offset=off),
                        f"duplicates path {path}")
            assert_same(ix.search_by_ids(dup + off, K), full, f"duplicates, self kept, path {path}")
        ix.set_path(PATH_AUTO)
        # ids repeated within one call
        rep = np.array([7, 7, 300, 7, 300, 2999, 0, 0])
        assert_same(ix.search_by_ids(rep + off, K, exclude_self=True), expect(O, pc, metric, rep, K, exclude_self=True, id_offset=off), "repeats")
        # a filter that leaves half of the query rows out: those rows are not in their own lists to begin with
        allow = np.random.default_rng(11).random(N) < 0.5
        q = np.arange(100, 140)
        assert 5 <= allow[q].sum() <= 35
        ix.set_filter(allow)
        for ex in (False, True):
            assert_same(ix.search_by_ids(q + off, K, exclude_self=ex), expect(O, pc, metric, q, K, elig=allow, exclude_self=ex, id_offset=off),
                        f"filter exclude {ex}")
        # k + 1 more than the eligible rows: the tail slots are unfilled
        few = np.zeros(N, bool)
        few[[5, 100, 101, 2000, 2999]] = True
        ix.set_filter(few)
        q = np.array([5, 100, 7, 2999, 1500])
        for ex in (False, True):
            got = ix.search_by_ids(q + off, K, exclude_self=ex)
            assert_same(got, expect(O, pc, metric, q, K, elig=few, exclude_self=ex, id_offset=off), f"few eligible, exclude {ex}")
            filled = (got[0] != ID_NONE).sum(axis=1).tolist()
            assert filled == ([4, 4, 5, 4, 5] if ex else [5] * 5)
        ix.set_filter(None)
        # the largest k the drop allows
        got = ix.search_by_ids(np.array([17]) + off, va.MAX_K - 1, exclude_self=True)
        assert_same(got, expect(O, pc, metric, [17], va.MAX_K - 1, exclude_self=True, id_offset=off), "k = MAX_K - 1")


# ------------------------------------------------------------------ after delete / update / compact
def raw_call(ix, ids, k, flags):
    ids = np.ascontiguousarray(ids, np.uint64)
    oi = np.full((ids.size, k), SENT_ID, np.uint64)
    sc = np.full((ids.size, k), SENT_SC, np.float32)
    rc = ix._L.vrod_search_by_ids(ix._h, ids.ctypes.data_as(C.c_void_p), ids.size, k, flags, oi.ctypes.data_as(C.c_void_p),
                                  sc.ctypes.data_as(C.c_void_p))
    return rc, oi, sc


@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2")])
def test_after_delete_update_and_compact(va, O, dtype, metric):
    d = 72
    base, _ = corpus(O, d, dtype, metric)
    raw = base.copy()
    rng = np.random.default_rng(21)
    dead = rng.choice(N, N // 10, replace=False)
    live = np.ones(N, bool)
    live[dead] = False
    upd = rng.choice(np.flatnonzero(live), 50, replace=False)
    new_rows = raw_corpus(50, d, metric, 77)
    with make_index(va, raw, dtype, metric) as ix:
        ix.delete(dead)
        ix.update(upd, new_rows)
        raw[upd] = new_rows
        pc = prepare(O, raw, dtype, metric)
        q = np.concatenate([upd[:20], rng.choice(np.flatnonzero(live), 60, replace=False)])
        for ex in (False, True):
            got = ix.search_by_ids(q, K, exclude_self=ex)
            assert_same(got, expect(O, pc, metric, q, K, elig=live, exclude_self=ex), f"mutated, exclude {ex}")
            assert not np.isin(got[0], dead.astype(np.uint64)).any()
        # a deleted id, an id past the rows: the whole call fails and nothing is written
        for bad in (dead[0], N, 1 << 40):
            rc, oi, sc = raw_call(ix, np.array([q[0], bad, q[1]]), K, 1)
            assert rc == 1 and (oi == SENT_ID).all() and (sc == SENT_SC).all(), bad
        new_ids = ix.compact()
        assert ix.count == live.sum()
        raw2 = np.ascontiguousarray(raw[live])
        pc2 = prepare(O, raw2, dtype, metric)
        q2 = new_ids[q].astype(np.int64)
        assert (new_ids[q] != ID_NONE).all()
        for ex in (False, True):
            assert_same(ix.search_by_ids(q2, K, exclude_self=ex), expect(O, pc2, metric, q2, K, exclude_self=ex), f"compacted, exclude {ex}")
        rc, oi, _ = raw_call(ix, np.array([int(live.sum())]), K, 0)
        assert rc == 1 and (oi == SENT_ID).all()


# ------------------------------------------------------------------ device form
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "ip")])
def test_device_form_matches_the_host_form(va, O, dtype, metric):
    import torch
    raw, pc = corpus(O, 72, dtype, metric)
    q = np.random.default_rng(5).choice(np.setdiff1d(np.arange(N), [11]), 40, replace=False)   # (row 11 is deleted below)
    dev = torch.device("cuda:0")
    with make_index(va, raw, dtype, metric) as ix:
        ix.delete([11])
        live = np.ones(N, bool)
        live[11] = False
        stream = torch.cuda.Stream(device=dev)
        for ex in (False, True):
            host = ix.search_by_ids(q, K, exclude_self=ex)
            with torch.cuda.stream(stream):
                d_ids = torch.from_numpy(q.astype(np.int64)).to(dev, non_blocking=True)
                oi = torch.full((q.size, K), 0x5A5A5A5A, dtype=torch.int64, device=dev)
                osc = torch.full((q.size, K), float(SENT_SC), dtype=torch.float32, device=dev)
                ix.search_by_ids_device(d_ids, K, exclude_self=ex, out_ids=oi, out_scores=osc)
            got = (oi.cpu().numpy().view(np.uint64), osc.cpu().numpy())
            assert_same(got, host, f"device form, exclude {ex}")
            assert_same(got, expect(O, pc, metric, q, K, elig=live, exclude_self=ex), f"device form against the oracle, exclude {ex}")
            # a bad id (past the rows, deleted): reported, the outputs keep what they held
            for bad in (N + 5, 11):
                with torch.cuda.stream(stream):
                    b_ids = torch.tensor([int(q[0]), bad, int(q[1])], dtype=torch.int64, device=dev)
                    oi.fill_(0x5A5A5A5A)
                    osc.fill_(float(SENT_SC))
                    with pytest.raises(va.VrodError) as e:
                        ix.search_by_ids_device(b_ids, K, exclude_self=ex, out_ids=oi, out_scores=osc)
                assert e.value.code == 1
                assert (oi.cpu().numpy() == 0x5A5A5A5A).all() and (osc.cpu().numpy() == SENT_SC).all()
            # ... and the handle is as usable as before
            assert_same(ix.search_by_ids(q, K, exclude_self=ex), host, "after a rejected call")


# ------------------------------------------------------------------ the graph
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2")])
def test_knn_graph(va, O, dtype, metric):
    d = 64
    batch = va.index.KNN_BATCH[DT[dtype]]
    n = 2 * batch + 300                              # three batches: both workspaces reused, a partial tail
    raw, pc = corpus(O, d, dtype, metric, n=n)
    allq = np.arange(n)
    want = expect(O, pc, metric, allq, K, exclude_self=True)
    with make_index(va, raw, dtype, metric) as ix:
        graph = ix.knn_graph(K)
        st = ix.last_stats()
        assert ix.pending == 0
        assert_same(ix.search_by_ids(allq, K, exclude_self=True), want, "by ids")
        assert_same(graph, want, "graph")
        assert st["nq"] == n and st["k"] == K and st["scan_launches"] >= 3, st
        assert st["scan_flops"] == sum(2.0 * m * n * d for m in (batch, batch, 300)), st
        # a sub-range that starts mid-batch
        first, m = batch // 2 + 3, batch + 77
        sub = ix.knn_graph(K, first_id=first, n=m)
        assert_same(sub, (want[0][first:first + m], want[1][first:first + m]), "sub-range")
        assert ix.last_stats()["nq"] == m
        assert ix.knn_graph(K, first_id=n, n=0)[0].shape == (0, K)
        with pytest.raises(va.VrodError) as e:
            ix.knn_graph(K, first_id=n - 5, n=6)
        assert e.value.code == 1
        # an ordinary search on the handle afterwards
        rq = raw_corpus(9, d, metric, 99)
        scan = METRIC_L2 if metric == "l2" else METRIC_COSINE
        assert_same(ix.search(rq, K), O.scan_topk(pc, prepare(O, rq, dtype, metric), K, scan, threads=THREADS), "ordinary search after the graph")

        # 5 % of the rows deleted, one whole stretch among them: deleted rows get unfilled rows, live rows the live rows
        rng = np.random.default_rng(31)
        dead = np.unique(np.concatenate([rng.choice(n, n // 20, replace=False), np.arange(batch + 10, batch + 40)]))
        live = np.ones(n, bool)
        live[dead] = False
        ix.delete(dead)
        g_ids, g_sc = ix.knn_graph(K)
        st = ix.last_stats()
        assert ix.pending == 0
        assert (g_ids[dead] == ID_NONE).all() and np.isnan(g_sc[dead]).all()
        lq = np.flatnonzero(live)
        assert_same((g_ids[lq], g_sc[lq]), expect(O, pc, metric, lq, K, elig=live, exclude_self=True), "graph with deletions")
        assert st["nq"] == lq.size, st
        assert st["scan_flops"] == sum(2.0 * live[b0:b0 + batch].sum() * n * d for b0 in range(0, n, batch)), st

        # a filter restricts the neighbours, not the queries
        allow = rng.random(n) < 0.3
        ix.set_filter(allow)
        f_ids, f_sc = ix.knn_graph(K)
        elig = live & allow
        assert_same((f_ids[lq], f_sc[lq]), expect(O, pc, metric, lq, K, elig=elig, exclude_self=True), "graph under a filter")
        assert (f_ids[dead] == ID_NONE).all()
        assert np.isin(f_ids[lq], np.flatnonzero(elig).astype(np.uint64)).all()
        ix.set_filter(None)

        # a batch whose every row is deleted is not searched at all
        ix.delete(np.arange(batch, 2 * batch))
        live[batch:2 * batch] = False
        g_ids, g_sc = ix.knn_graph(K)
        lq = np.flatnonzero(live)
        assert (g_ids[~live] == ID_NONE).all() and np.isnan(g_sc[~live]).all()
        assert_same((g_ids[lq], g_sc[lq]), expect(O, pc, metric, lq, K, elig=live, exclude_self=True), "graph with an empty batch")
        assert ix.last_stats()["nq"] == lq.size and ix.pending == 0


# ------------------------------------------------------------------ flags and the k limit on a live handle
def test_flag_bits_and_k_limit_on_a_live_handle(va, O):
    import torch
    raw, pc = corpus(O, 72, "bf16", "cosine")
    dev = torch.device("cuda:0")
    big = va.MAX_K
    with make_index(va, raw, "bf16", "cosine") as ix:
        d_ids = torch.tensor([1, 2], dtype=torch.int64, device=dev)
        d_oi = torch.full((2, big), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        d_sc = torch.full((2, big), float(SENT_SC), dtype=torch.float32, device=dev)

        def device_call(k, flags):
            rc = ix._L.vrod_search_by_ids_device(ix._h, d_ids.data_ptr(), 2, k, flags, d_oi.data_ptr(), d_sc.data_ptr(), None)
            return rc, d_oi.cpu().numpy(), d_sc.cpu().numpy()

        for k, flags in ((K, 2), (K, 0x80000001), (K, 0xFFFFFFFE), (big, 1), (big + 1, 0), (big + 1, 1), (0, 0), (0, 1)):
            rc, oi, sc = raw_call(ix, np.array([1, 2]), k, flags)          # (buffers of [2, k]: nothing may be written)
            assert rc == 1 and (oi == SENT_ID).all() and (sc == SENT_SC).all(), (k, flags)
            if k <= big:                                                     # (the device buffers hold [2, MAX_K])
                rc, oi, sc = device_call(k, flags)
                assert rc == 1 and (oi == 0x5A5A5A5A).all() and (sc == SENT_SC).all(), (k, flags)
        # the graph: its k stops at MAX_K - 1
        g_ids = np.full((4, big), SENT_ID, np.uint64)
        g_sc = np.full((4, big), SENT_SC, np.float32)
        for k in (big, 0):
            rc = ix._L.vrod_knn_graph(ix._h, 0, 4, k, g_ids.ctypes.data_as(C.c_void_p), g_sc.ctypes.data_as(C.c_void_p))
            assert rc == 1 and (g_ids == SENT_ID).all() and (g_sc == SENT_SC).all(), k
        assert ix.pending == 0
        # k = MAX_K without the flag is fine, on both forms; so is MAX_K - 1 with it, graph included
        want = expect(O, pc, "cosine", [1, 2], big)
        assert_same(ix.search_by_ids([1, 2], big), want, "k = MAX_K, self kept")
        rc, oi, sc = device_call(big, 0)
        assert rc == 0
        assert_same((oi.view(np.uint64), sc), want, "k = MAX_K, self kept, device form")
        assert_same(ix.knn_graph(big - 1, first_id=0, n=4), expect(O, pc, "cosine", np.arange(4), big - 1, exclude_self=True), "graph at k = MAX_K - 1")


# ------------------------------------------------------------------ interlock, multi-device
def test_pending_search_blocks_all_three_entry_points(va, O):
    import torch
    raw, pc = corpus(O, 72, "bf16", "cosine")
    dev = torch.device("cuda:0")
    with make_index(va, raw, "bf16", "cosine") as ix:
        dq = torch.from_numpy(raw[:4].copy()).to(dev)
        oi = torch.empty((4, K), dtype=torch.int64, device=dev)
        osc = torch.empty((4, K), dtype=torch.float32, device=dev)
        ix.search_begin_device(dq, K, oi, osc)
        assert ix.pending == 1
        rc, hi, hs = raw_call(ix, np.array([1, 2]), K, 1)
        assert rc == 1 and (hi == SENT_ID).all() and (hs == SENT_SC).all()
        d_ids = torch.tensor([1, 2], dtype=torch.int64, device=dev)
        with pytest.raises(va.VrodError) as e:
            ix.search_by_ids_device(d_ids, K)
        assert e.value.code == 1
        with pytest.raises(va.VrodError) as e:
            ix.knn_graph(K, first_id=0, n=8)
        assert e.value.code == 1
        assert ix.pending == 1
        ix.search_end()
        assert_same(ix.search_by_ids([1, 2], K, exclude_self=True), expect(O, pc, "cosine", [1, 2], K, exclude_self=True), "after the pending search")


def test_multi_device_handle_is_unsupported(va, O):
    import torch
    raw, _ = corpus(O, 72, "bf16", "cosine")
    dev = torch.device("cuda:0")
    with va.Index(72, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        rc, hi, hs = raw_call(ix, np.array([1, 2]), K, 0)
        assert rc == 6 and (hi == SENT_ID).all() and (hs == SENT_SC).all()
        d_ids = torch.tensor([1, 2], dtype=torch.int64, device=dev)
        oi = torch.full((2, K), 0x5A5A5A5A, dtype=torch.int64, device=dev)
        osc = torch.full((2, K), float(SENT_SC), dtype=torch.float32, device=dev)
        with pytest.raises(va.VrodError) as e:
            ix.search_by_ids_device(d_ids, K, out_ids=oi, out_scores=osc)
        assert e.value.code == 6 and (oi.cpu().numpy() == 0x5A5A5A5A).all() and (osc.cpu().numpy() == SENT_SC).all()
        g_ids = np.full((8, K), SENT_ID, np.uint64)
        g_sc = np.full((8, K), SENT_SC, np.float32)
        rc = ix._L.vrod_knn_graph(ix._h, 0, 8, K, g_ids.ctypes.data_as(C.c_void_p), g_sc.ctypes.data_as(C.c_void_p))
        assert rc == 6 and (g_ids == SENT_ID).all() and (g_sc == SENT_SC).all()
