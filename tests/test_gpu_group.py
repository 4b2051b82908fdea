"""GPU tests of the grouped search (vrod_search_grouped) against the CPU oracle.

The contract: every label carried by an eligible row (live, allowed) has one representative, its best eligible row; query
q's result row is the k best representatives, best first, ties by smaller id, a NaN score last, padded with
(ID_NONE, NaN, label 0).  The expected values come from the oracle alone: per label the oracle's top-1 over that label's
eligible rows (taken in ascending order, so ties break by the smaller id), ordered with numpy, cut to k.

One corpus of 20 000 Gaussian rows (d = 64, and d = 100 whose tail chunk is padded) with planted structure:
  - 300 labels of about 20 rows, labels of exactly 1, 63, 64 and 65 rows, label 0 on what is left;
  - a heavy label A whose 5 000 rows are small perturbations of query 0, and a heavy label B whose 3 700 rows are small
    perturbations of query 1, itself a perturbation of query 0: for query 1 the best ranks are B's rows, then A's, so
    with k = 3 the first list is all B, the first dense round all A, and only the second dense round finds a third
    label;
  - a broad label on 4 500 rows.  (A label on half of the rows does not fit: the heavy labels need more than VROD_MAX_K
    rows each and the 300 small labels 6 000, so the broad label takes the largest share that is left.)
Queries 0 and 1 are "heavy" (their best ranks belong to A and B: the candidate search cannot find k >= 3 labels and the
dense stage finishes them), queries 2 .. 69 are "light".  Both premises are asserted from the oracle's full ranking
before the library is asked anything:
  - the best VROD_MAX_K ranks of a heavy query hold at most 2 labels, and query 1's two-round structure is as described;
  - for k = 1 and k = 10 (the k of the fallback-count checks) every light query has k distinct labels within the first
    k1 = max(4 k, k + 32) ranks.  For k = 300 that cannot hold on this corpus -- 1 200 ranks of Gaussian rows hold about
    210 of its ~ 310 labels -- so at k = 300 and k = 400 light queries take the dense stage too, which the comparison
    with the oracle covers.
"""
import numpy as np
import pytest

import support
from support import (  # noqa: F401
    DT, METRIC_COSINE, METRIC_L2, PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, MAX_K, THREADS, va, O, bits, first_k)

pytestmark = pytest.mark.gpu

N, NQ = 20_000, 70
L_A, L_B, L_BROAD = 3_000_000_000, 70_000, 0xFFFFFFFF
N_A, N_B, N_BROAD = 5_000, 3_700, 4_500
L_EXACT = {1: 1, 63: 63, 64: 64, 65: 65}          # label -> rows
SMALL0, N_SMALL = 10_000, 300
HEAVY = (0, 1)
K_ABOVE = 400                                      # more than the corpus has labels


def assert_same(got, want, what=""):
    (ids, sc, lab), (oi, osc, ol) = got, want
    support.assert_same(ids, sc, oi, osc, what)
    assert np.array_equal(lab, ol), f"{what}: labels differ at {np.argwhere(lab != ol)[:5]}"


def prepared(O, raw, rq, dtype, metric):
    prep = METRIC_COSINE if metric == "cosine" else METRIC_L2
    return O.prepare(raw, DT[dtype], prep, threads=THREADS), O.prepare(rq, DT[dtype], prep, threads=THREADS)


def representatives(O, raw, rq, dtype, metric, labels, ok=None, id_offset=0):
    """Per query every label's representative, best first: (ids, scores, labels), each [nq, distinct labels].
    The oracle's top-1 over each label's eligible rows in ascending order; the order among them is numpy's."""
    ok = np.ones(labels.size, bool) if ok is None else ok
    scan = METRIC_L2 if metric == "l2" else METRIC_COSINE
    pc, pq = prepared(O, raw, rq, dtype, metric)
    present = np.unique(labels[ok])
    nq = rq.shape[0]
    ids = np.empty((nq, present.size), np.uint64)
    sc = np.empty((nq, present.size), np.float32)
    for j, L in enumerate(present):
        rows = np.flatnonzero((labels == L) & ok)
        i, s = O.scan_topk(np.ascontiguousarray(pc[rows]), pq, 1, scan, threads=THREADS)
        ids[:, j] = rows[i[:, 0].astype(np.int64)].astype(np.uint64) + np.uint64(id_offset)
        sc[:, j] = s[:, 0]
    lab = np.broadcast_to(present.astype(np.uint32), ids.shape).copy()
    for q in range(nq):
        nan = np.isnan(sc[q])
        val = np.where(nan, np.float32(0), sc[q] if scan == METRIC_L2 else -sc[q])
        o = np.lexsort((ids[q], val, nan))                      # NaN last, then the score, then the id
        ids[q], sc[q], lab[q] = ids[q][o], sc[q][o], lab[q][o]
    return ids, sc, lab


def cut(reps, nq, k):
    ids, sc, lab = (a[:nq] for a in reps)
    oi = np.full((nq, k), ID_NONE, np.uint64)
    osc = np.full((nq, k), np.nan, np.float32)
    ol = np.zeros((nq, k), np.uint32)
    m = min(k, ids.shape[1])
    oi[:, :m], osc[:, :m], ol[:, :m] = ids[:, :m], sc[:, :m], lab[:, :m]
    return oi, osc, ol


def make_labels(rng):
    lab = np.zeros(N, np.uint32)
    perm = rng.permutation(N)
    at = 0
    where = {}

    def take(n, value):
        nonlocal at
        lab[perm[at:at + n]] = value
        where[value] = np.sort(perm[at:at + n])
        at += n
    take(N_A, L_A)
    take(N_B, L_B)
    take(N_BROAD, L_BROAD)
    for value, n in L_EXACT.items():
        take(n, value)
    sizes = rng.integers(14, 27, N_SMALL)
    for j in range(N_SMALL):
        take(int(sizes[j]), SMALL0 + j)
    assert at < N                                  # the rest keeps label 0
    return lab, where


SEED = 20267                                       # (a seed for which the premises below hold; they are asserted)


@pytest.fixture(scope="module")
def world():
    return make_world(SEED)


def make_world(seed):
    rng = np.random.default_rng(seed)
    labels, where = make_labels(rng)
    corpora, queries = {}, {}
    for d in (64, 100):
        raw = rng.standard_normal((N, d)).astype(np.float32)
        rq = rng.standard_normal((NQ, d)).astype(np.float32)
        rq[1] = rq[0] + 0.5 * rng.standard_normal(d).astype(np.float32)
        raw[where[L_A]] = rq[0] + 0.05 * rng.standard_normal((N_A, d)).astype(np.float32)
        raw[where[L_B]] = rq[1] + 0.05 * rng.standard_normal((N_B, d)).astype(np.float32)
        corpora[d], queries[d] = raw, rq
    return labels, corpora, queries


def check_premises(O, raw, rq, dtype, metric, labels, what):
    """From the oracle's full ranking: the heavy queries are heavy, the light ones light (module docstring)."""
    scan = METRIC_L2 if metric == "l2" else METRIC_COSINE
    pc, pq = prepared(O, raw, rq, dtype, metric)
    deep = MAX_K + first_k(3, N) + 200                           # B's rows and one more list, for the heavy queries
    order, _ = O.scan_topk(pc, np.ascontiguousarray(pq[list(HEAVY)]), deep, scan, threads=THREADS)
    ranked = labels[order.astype(np.int64)]                      # [heavy query, rank]: the label at every rank
    for j, q in enumerate(HEAVY):
        owners = np.unique(ranked[j, :MAX_K])
        assert owners.size <= 2 and set(owners) <= {L_A, L_B}, f"{what}: query {q} is not heavy: {owners[:8]}"
    k1 = first_k(3, N)
    assert set(ranked[1, :k1]) == {L_B}, f"{what}: query 1's first list is not all B"
    rest = ranked[1][ranked[1] != L_B]
    assert rest.size >= k1 and set(rest[:k1]) == {L_A}, f"{what}: query 1's first dense round is not all A"
    order, _ = O.scan_topk(pc, np.ascontiguousarray(pq[len(HEAVY):]), first_k(10, N), scan, threads=THREADS)
    ranked = labels[order.astype(np.int64)]
    for k in (1, 10):
        k1 = first_k(k, N)
        for q in range(ranked.shape[0]):
            assert np.unique(ranked[q, :k1]).size >= k, f"{what}: light query {q + len(HEAVY)} needs more than {k1} ranks for k={k}"


# ---------------------------------------------------------------- every dtype x metric, AUTO and EXACT, every nq and k
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [64, 100])
def test_grouped_matches_the_oracle(va, O, world, dim, dtype, metric):
    labels, corpora, queries = world
    raw, rq = corpora[dim], queries[dim]
    tag = f"{dim}/{dtype}/{metric}"
    check_premises(O, raw, rq, dtype, metric, labels, tag)
    reps = representatives(O, raw, rq, dtype, metric, labels)
    n_labels = reps[0].shape[1]
    assert 300 < n_labels < K_ABOVE
    light = np.ascontiguousarray(rq[2:])
    light_reps = tuple(a[2:] for a in reps)
    rb = (-(-dim // 64) * 64 * 2) if dtype == "bf16" else (-(-dim // 32) * 32 * 4)
    with va.Index(dim, dtype, metric) as ix:
        ix.add(raw)
        ix.set_labels(0, labels)
        for path in (PATH_AUTO, PATH_EXACT):
            ix.set_path(path)
            for nq in (1, 7, NQ):
                n_heavy = min(nq, len(HEAVY))
                for k in (1, 3, 10, 300, K_ABOVE):
                    what = f"{tag}/path{path}/nq{nq}/k{k}"
                    pinned = path == PATH_AUTO and k == 10
                    if pinned:
                        # A handle adapts its plan to failed certificates: the candidate margin of a batched search doubles
                        # after a search in which some failed and is reset and held once it reaches 8 (four steps), and an
                        # fp32 handle gives up its split pass after two searches in which many failed.  Eight runs of the
                        # very search the candidate stage is going to make leave the handle where that search no longer
                        # moves it, so that the grouped search and the plain search after it run the same plan.
                        for _ in range(8):
                            ix.search(rq[:nq], first_k(k, N))
                    got = ix.search_grouped(rq[:nq], k)
                    st = ix.last_stats()
                    print(what, st)
                    assert_same(got, cut(reps, nq, k), what)
                    assert st["nq"] == nq and st["k"] == k, f"{what}: {st}"
                    if k == K_ABOVE:
                        assert (got[0][:, n_labels:] == ID_NONE).all() and (got[0][:, :n_labels] != ID_NONE).all()
                        assert not got[2][:, n_labels:].any()
                    if path == PATH_EXACT:
                        passes = nq // 8 + bin(nq % 8).count("1")          # groups of 8, then of 4, 2, 1 queries
                        assert st["path"] == PATH_EXACT and st["fallback_queries"] == nq and st["kprime"] == 0, f"{what}: {st}"
                        assert st["scan_bytes"] == passes * N * rb and st["scan_launches"] == passes, f"{what}: {st}"
                        assert st["scan_flops"] == 2.0 * nq * N * dim, f"{what}: {st}"
                    elif pinned:
                        # the heavy queries, and only they, took the dense stage (one pass: they are at most 2): every
                        # counter is the candidate search's own -- the same search, run plainly -- plus that
                        ix.search(rq[:nq], first_k(k, N))
                        plain = ix.last_stats()
                        print(what, "plain", plain)
                        assert st["fallback_queries"] == plain["fallback_queries"] + n_heavy, f"{what}: {st} {plain}"
                        assert st["kprime"] == plain["kprime"] and st["kprime"] >= first_k(k, N), f"{what}: {st} {plain}"
                        assert st["scan_bytes"] == plain["scan_bytes"] + N * rb, f"{what}: {st} {plain}"
                        assert st["scan_flops"] == plain["scan_flops"] + 2.0 * n_heavy * N * dim, f"{what}: {st} {plain}"
                        assert st["scan_launches"] == plain["scan_launches"] + 1, f"{what}: {st} {plain}"
                        assert st["path"] == (PATH_EXACT if nq == n_heavy else plain["path"]), f"{what}: {st} {plain}"
                        # the three batch sizes are three first stages: stream, the skinny batched form (<= 64 queries
                        # over bf16 rows; an fp32 handle may still stream 7 queries), the tiled batched form
                        want = {1: (PATH_STREAM,), 7: (PATH_MFMA,) if dtype == "bf16" else (PATH_STREAM, PATH_MFMA), NQ: (PATH_MFMA,)}[nq]
                        assert plain["path"] in want, f"{what}: {plain}"
                    elif k == 1:
                        assert st["path"] != PATH_EXACT, f"{what}: {st}"      # one label is always found: no dense stage
            if path == PATH_AUTO:
                for nq in (7, NQ - 2):                                        # all-light batches: only the candidate search
                    for k in (1, 10):
                        what = f"{tag}/light/nq{nq}/k{k}"
                        got = ix.search_grouped(light[:nq], k)
                        st = ix.last_stats()
                        ix.search(light[:nq], first_k(k, N))
                        plain = ix.last_stats()
                        print(what, st, plain["fallback_queries"])
                        assert_same(got, cut(light_reps, nq, k), what)
                        assert st["fallback_queries"] == plain["fallback_queries"] and st["path"] == plain["path"], f"{what}: {st} {plain}"
                        assert st["scan_bytes"] == plain["scan_bytes"] and st["scan_flops"] == plain["scan_flops"], f"{what}: {st} {plain}"
                        assert st["kprime"] == plain["kprime"], f"{what}: {st} {plain}"


# ---------------------------------------------------------------- a small corpus of its own for the remaining cases
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(31)
    n, dim = 6_000, 64
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    labels = (rng.permutation(n) % 40 + 100).astype(np.uint32)          # 40 labels of 150 rows
    rq = rng.standard_normal((9, dim)).astype(np.float32)
    return raw, labels, rq


def test_exact_duplicates_tie_by_id(va, O, small):
    raw, labels, rq = (a.copy() for a in small)
    dup = [17, 400, 401, 2222, 3000, 3001, 4500, 5999]                  # ascending ids, labels 9 down to 2
    raw[dup] = rq[0]
    labels[dup] = np.arange(9, 1, -1, dtype=np.uint32)
    for dtype, metric in (("f32", "cosine"), ("bf16", "l2"), ("bf16", "ip")):
        reps = representatives(O, raw, rq, dtype, metric, labels)
        with va.Index(64, dtype, metric) as ix:
            ix.add(raw)
            ix.set_labels(0, labels)
            for path in (PATH_AUTO, PATH_EXACT):
                ix.set_path(path)
                for k in (3, 8, 20):
                    got = ix.search_grouped(rq, k)
                    assert_same(got, cut(reps, 9, k), f"{dtype}/{metric}/path{path}/k{k}")
                    if metric != "ip":                                   # (an inner product has no reason to prefer the copy)
                        m = min(k, 8)
                        assert got[0][0, :m].tolist() == dup[:m] and got[2][0, :m].tolist() == list(range(9, 9 - m, -1))


@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "l2")])
def test_filter_delete_update_compact(va, O, small, dtype, metric):
    raw, labels, rq = (a.copy() for a in small)
    n, k, off = raw.shape[0], 12, 1_000_000
    rng = np.random.default_rng(8)
    with va.Index(64, dtype, metric) as ix:
        ix.add(raw)
        ix.set_id_offset(off)
        ix.set_labels(off, labels)
        reps = representatives(O, raw, rq, dtype, metric, labels, None, off)
        assert_same(ix.search_grouped(rq, k), cut(reps, 9, k), "plain")
        # a filter that removes the best row of query 0's best label (and a random third of the rows): the representative changes
        best_id, best_label = int(reps[0][0, 0]) - off, int(reps[2][0, 0])
        allow = rng.random(n) < 0.67
        allow[best_id] = False
        others = np.flatnonzero(labels == best_label)
        allow[others[others != best_id][-1]] = True                      # (the label keeps an eligible row)
        ix.set_filter(allow)
        reps_f = representatives(O, raw, rq, dtype, metric, labels, allow, off)
        j = int(np.flatnonzero(reps_f[2][0] == best_label)[0])
        assert int(reps_f[0][0, j]) != best_id + off
        for path in (PATH_AUTO, PATH_EXACT, PATH_GATHER):
            ix.set_path(path)
            assert_same(ix.search_grouped(rq, k), cut(reps_f, 9, k), f"filter path{path}")
            assert_same(ix.search_grouped(rq, 64), cut(reps_f, 9, 64), f"filter path{path} k above the labels")
        ix.set_path(PATH_AUTO)
        # a whole label deleted: gone from the result
        dead = np.flatnonzero(labels == best_label)
        ix.delete(dead + off)
        ok = allow.copy()
        ok[dead] = False
        reps_d = representatives(O, raw, rq, dtype, metric, labels, ok, off)
        got = ix.search_grouped(rq, 64)
        assert_same(got, cut(reps_d, 9, 64), "after delete")
        assert best_label not in got[2][got[0] != ID_NONE] and (got[0][:, 39:] == ID_NONE).all() and (got[0][:, :39] != ID_NONE).all()
        # a representative updated to a far-away vector: another row of its label takes over
        rep_id, rep_label = int(reps_d[0][1, 0]) - off, int(reps_d[2][1, 0])
        raw[rep_id] = -rq[1] if metric == "cosine" else rq[1] + 100.0
        ix.update(np.array([rep_id + off], np.uint64), raw[rep_id:rep_id + 1])
        reps_u = representatives(O, raw, rq, dtype, metric, labels, ok, off)
        j = int(np.flatnonzero(reps_u[2][1] == rep_label)[0])
        assert int(reps_u[0][1, j]) != rep_id + off
        for path in (PATH_AUTO, PATH_EXACT):
            ix.set_path(path)
            assert_same(ix.search_grouped(rq, k), cut(reps_u, 9, k), f"after update path{path}")
        ix.set_path(PATH_AUTO)
        # compact: new ids, same labels
        live = np.setdiff1d(np.arange(n), dead)
        ix.compact()
        assert ix.count == live.size
        reps_c = representatives(O, raw[live], rq, dtype, metric, labels[live], allow[live], off)
        got = ix.search_grouped(rq, k)
        assert_same(got, cut(reps_c, 9, k), "after compact")
        assert np.array_equal(got[2], cut(reps_u, 9, k)[2])               # the same labels as before, under new ids


def test_unset_labels_give_one_result(va, O, small):
    raw, _, rq = small
    reps = representatives(O, raw, rq, "bf16", "cosine", np.zeros(raw.shape[0], np.uint32))
    assert reps[0].shape == (9, 1)
    with va.Index(64, "bf16", "cosine") as ix:
        ix.add(raw)
        for path in (PATH_AUTO, PATH_EXACT):
            ix.set_path(path)
            got = ix.search_grouped(rq, 5)
            assert_same(got, cut(reps, 9, 5), f"unset labels path{path}")
            assert (got[0][:, 0] != ID_NONE).all() and (got[0][:, 1:] == ID_NONE).all()


def test_large_k_resolved_by_the_candidate_stage(va, O, small):
    """Few large labels at k = 30, and 2 000 labels of 3 rows at k = 900 (k1 = VROD_MAX_K: the de-duplication's table at
    its largest, 8 192 slots): the lists hold k distinct labels, so under AUTO nothing goes to the dense stage.  Both
    premises are asserted from the oracle's ranking."""
    raw, labels, rq = small
    n = raw.shape[0]
    many = (np.random.default_rng(32).permutation(n) % 2000).astype(np.uint32)
    pc, pq = prepared(O, raw, rq, "bf16", "cosine")
    order, _ = O.scan_topk(pc, pq, MAX_K, METRIC_COSINE, threads=THREADS)
    for lab, k in ((labels, 30), (many, 900)):
        k1 = first_k(k, n)
        assert k1 == (120 if k == 30 else MAX_K)
        assert all(np.unique(lab[order[q, :k1].astype(np.int64)]).size >= k for q in range(9)), f"k={k}: a list lacks k labels"
        reps = representatives(O, raw, rq, "bf16", "cosine", lab)
        with va.Index(64, "bf16", "cosine") as ix:
            ix.add(raw)
            ix.set_labels(0, lab)
            for _ in range(8):                                           # (settles the adaptive candidate margin)
                ix.search(rq, k1)
            got = ix.search_grouped(rq, k)
            st = ix.last_stats()
            ix.search(rq, k1)
            plain = ix.last_stats()
            print(k, st, plain)
            assert_same(got, cut(reps, 9, k), f"k={k}")
            assert (got[0] != ID_NONE).all()
            for f in ("path", "kprime", "fallback_queries", "scan_bytes", "scan_flops", "scan_launches"):
                assert st[f] == plain[f], f"k={k} {f}: {st} {plain}"
            ix.set_path(PATH_EXACT)
            assert_same(ix.search_grouped(rq, k), cut(reps, 9, k), f"k={k} exact")


def test_arguments_pending_and_multi_device(va, small):
    import ctypes as C
    import torch
    raw, labels, rq = small
    k = 4
    with va.Index(64, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_labels(0, labels)
        want = ix.search_grouped(rq, k)
        for bad_k in (0, MAX_K + 1):
            with pytest.raises(va.VrodError) as e:
                ix.search_grouped(rq, bad_k)
            assert e.value.code == 1
        L = ix._L
        q = np.ascontiguousarray(rq)
        ids, sc = np.empty((9, k), np.uint64), np.empty((9, k), np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
        assert L.vrod_search_grouped(ix._h, None, 9, k, vp(ids), vp(sc), None) == 1
        assert L.vrod_search_grouped(ix._h, vp(q), 9, k, None, vp(sc), None) == 1
        assert L.vrod_search_grouped(ix._h, vp(q), 9, k, vp(ids), None, None) == 1
        assert L.vrod_search_grouped(ix._h, vp(q), 9, k, vp(ids), vp(sc), None) == 0      # no labels wanted
        assert np.array_equal(ids, want[0]) and np.array_equal(bits(sc), bits(want[1]))
        nan = rq.copy()
        nan[4, 7] = np.inf
        for path in (PATH_AUTO, PATH_EXACT):
            ix.set_path(path)
            with pytest.raises(va.VrodError) as e:
                ix.search_grouped(nan, k)
            assert e.value.code == 2
        ix.set_path(PATH_AUTO)
        assert_same(ix.search_grouped(rq, k), want, "after rejected calls")
        # a pending search blocks the call; after search_end it works
        dq = torch.from_numpy(rq).cuda()
        oi = torch.empty((9, k), dtype=torch.int64, device="cuda")
        osc = torch.empty((9, k), dtype=torch.float32, device="cuda")
        ix.search_begin_device(dq, k, oi, osc)
        for call in (lambda: ix.search_grouped(rq, k), lambda: ix.search_grouped_device(dq, k)):
            with pytest.raises(va.VrodError) as e:
                call()
            assert e.value.code == 1
        ix.search_end()
        # the device form, with and without a label buffer
        di, ds, dl = ix.search_grouped_device(dq, k)
        assert_same((di.cpu().numpy().view(np.uint64), ds.cpu().numpy(), dl.cpu().numpy().view(np.uint32)), want, "device form")
        ix.set_path(PATH_EXACT)
        di, ds, dl = ix.search_grouped_device(dq, k, want_labels=False)
        assert dl is None
        assert np.array_equal(di.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(bits(ds.cpu().numpy()), bits(want[1]))
    with va.Index(64, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        ids, sc, lab = np.full((9, k), 7, np.uint64), np.full((9, k), 7, np.float32), np.full((9, k), 7, np.uint32)
        assert ix._L.vrod_search_grouped(ix._h, vp(q), 9, k, vp(ids), vp(sc), vp(lab)) == 6
        assert (ids == 7).all() and (sc == 7).all() and (lab == 7).all()
        with pytest.raises(va.VrodError) as e:
            ix.search_grouped(rq, k)
        assert e.value.code == 6
