"""GPU tests of row labels and the labelled search (vrod_index_set_labels / vrod_search_labeled) against the CPU oracle.

The contract: query q of a labelled search gets, bit for bit, what the oracle returns over the rows that are live,
allowed and labelled labels[q] -- scan_topk(prepared[those rows], ...), ids mapped back.  The rows of a label are taken
in ascending order, so ties still break by the smaller id; slots beyond them are (ID_NONE, NaN).

One corpus (40 000 rows; d = 64, and d = 100 whose tail chunk has padding that must not be walked) holds a label on half
of the rows (AUTO scans it densely), one on a tenth, labels of exactly 1, 63, 64, 65 and 8 193 (= kSelectChunk + 1) rows,
200 labels of ~20 rows, label 0 on what is left, and two labels no row carries.
"""
import numpy as np
import pytest

from support import (  # noqa: F401
    PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, va, O, assert_same, oracle_over, row_bytes, takes_segments)

pytestmark = pytest.mark.gpu

N = 40_000
L_HALF, L_TENTH, L_BIG, L_NONE_A, L_NONE_B = 4_000_000_000, 1000, 8193, 5, 77777
L_EXACT = {1: 1, 63: 63, 64: 64, 65: 65}          # label -> rows
SMALL0, N_SMALL = 10_000, 200


def expected(O, raw, rq, qlabels, k, dtype, metric, labels, ok=None, id_offset=0):
    """Per distinct query label, the oracle over the rows that carry it (and are `ok`: live and allowed)."""
    qlabels = np.asarray(qlabels, dtype=np.uint64)
    ids = np.empty((rq.shape[0], k), np.uint64)
    sc = np.empty((rq.shape[0], k), np.float32)
    ok = np.ones(labels.size, bool) if ok is None else ok
    for L in np.unique(qlabels):
        qs = np.flatnonzero(qlabels == L)
        rows = np.flatnonzero((labels == L) & ok)
        ids[qs], sc[qs] = oracle_over(O, raw, np.ascontiguousarray(rq[qs]), k, dtype, metric, rows, id_offset)
    return ids, sc


def make_labels(rng):
    lab = np.zeros(N, np.uint32)
    perm = rng.permutation(N)
    at = 0

    def take(n, value):
        nonlocal at
        lab[perm[at:at + n]] = value
        at += n
    take(N // 2, L_HALF)
    take(N // 10, L_TENTH)
    take(8193, L_BIG)
    for value, n in L_EXACT.items():
        take(n, value)
    sizes = rng.integers(12, 29, N_SMALL)
    for j in range(N_SMALL):
        take(int(sizes[j]), SMALL0 + j)
    assert at < N                                  # the rest keeps label 0
    return lab


def query_labels(rng, nq):
    if nq == 1:
        return np.array([L_TENTH], np.uint32)
    if nq == 9:
        return np.array([L_HALF, L_TENTH, 65, L_BIG, 1, L_NONE_B, SMALL0 + 3, SMALL0 + 3, SMALL0 + 150], np.uint32)
    q = [L_HALF] * 256 + [65] * 9 + [L_TENTH] * 3 + [1, 63, 64, L_BIG, L_BIG, L_NONE_A, L_NONE_B, 0]
    q += [SMALL0 + int(j) for j in rng.integers(0, N_SMALL, nq - len(q))]
    q = np.array(q, np.uint64)
    rng.shuffle(q)
    return q.astype(np.uint32)


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20261)
    labels = make_labels(rng)
    corpora = {d: rng.standard_normal((N, d)).astype(np.float32) for d in (64, 100)}
    queries = {d: rng.standard_normal((300, d)).astype(np.float32) for d in (64, 100)}
    qlabels = {nq: query_labels(rng, nq) for nq in (1, 9, 300)}
    return labels, corpora, queries, qlabels


def check_stats(st, path, dtype, dim, labels, ql, k, what):
    nq = len(ql)
    assert st["nq"] == nq and st["k"] == k, f"{what}: {st}"
    rb = row_bytes(dtype, dim)
    want_bytes = want_flops = 0.0
    any_dense = False
    for L in np.unique(ql):
        m, nqg = int((labels == L).sum()), int((ql == L).sum())
        if takes_segments(path, dtype, N, m, nqg, dim):
            want_bytes += m * rb
            want_flops += 2.0 * nqg * m * dim
        else:
            any_dense = True
            want_bytes += N * rb
            want_flops += 2.0 * nqg * N * dim
    assert st["scan_bytes"] == want_bytes and st["scan_flops"] == want_flops, f"{what}: {st} want {want_bytes} {want_flops}"
    if not any_dense:
        assert st["path"] == PATH_GATHER and st["kprime"] == 0, f"{what}: {st}"
        assert st["max_fast_err"] == 0 and st["eps_bound"] == 0 and st["fallback_queries"] == 0 and st["band_queries"] == 0, f"{what}: {st}"
    else:
        assert st["path"] != PATH_GATHER, f"{what}: {st}"
        if path != PATH_AUTO:
            assert st["path"] == path, f"{what}: {st}"
        if st["path"] != PATH_EXACT and np.isfinite(st["eps_bound"]):
            assert st["max_fast_err"] <= st["eps_bound"], f"{what}: {st}"
    return any_dense


# ---------------------------------------------------------------- every route x dtype x metric
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [64, 100])
def test_every_route(va, O, world, dim, dtype, metric):
    labels, corpora, queries, qlabels = world
    raw, k = corpora[dim], 10
    want = {nq: expected(O, raw, queries[dim][:nq], qlabels[nq], k, dtype, metric, labels) for nq in (1, 9, 300)}
    with va.Index(dim, dtype, metric) as ix:
        ix.add(raw)
        ix.set_labels(0, labels)
        assert np.array_equal(ix.get_labels(0, N), labels)
        for path in (PATH_GATHER, PATH_MFMA, PATH_EXACT, PATH_STREAM, PATH_AUTO):
            ix.set_path(path)
            for nq in (1, 9, 300):
                what = f"{dim}/{dtype}/{metric}/path{path}/nq{nq}"
                ids, sc = ix.search_labeled(queries[dim][:nq], k, qlabels[nq])
                st = ix.last_stats()
                print(what, st)
                assert_same(ids, sc, *want[nq], what)
                check_stats(st, path, dtype, dim, labels, qlabels[nq], k, what)
                if path == PATH_AUTO and nq == 300:
                    assert st["path"] == PATH_MFMA, f"{what}: {st}"      # the 50 % label, 256 queries: a batched scan


# ---------------------------------------------------------------- launch count
def test_launch_count_does_not_grow_with_labels(va, O):
    rng = np.random.default_rng(77)
    n, dim, k = 20_000, 64, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((256, dim)).astype(np.float32)
    launches = {}
    for n_labels, ql in ((256, rng.permutation(256).astype(np.uint32)), (4, rng.integers(0, 4, 256).astype(np.uint32))):
        labels = (rng.permutation(n) % n_labels).astype(np.uint32)       # n_labels labels, n rows in all
        with va.Index(dim, "bf16", "cosine") as ix:
            ix.add(raw)
            ix.set_labels(0, labels)
            ix.set_path(PATH_GATHER)
            ids, sc = ix.search_labeled(rq, k, ql)
            st = ix.last_stats()
        print(n_labels, st)
        assert_same(ids, sc, *expected(O, raw, rq, ql, k, "bf16", "cosine", labels), f"{n_labels} labels")
        assert st["path"] == PATH_GATHER
        launches[n_labels] = st["scan_launches"]
    assert launches[256] == launches[4] and 1 <= launches[256] <= 2, launches


# ---------------------------------------------------------------- ties by id
@pytest.mark.parametrize("path", [PATH_GATHER, PATH_AUTO, PATH_MFMA])
def test_ties_break_by_id_within_a_label(va, O, path):
    rng = np.random.default_rng(5)
    n, dim = 6_000, 64
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    labels = (np.arange(n) % 3 + 1).astype(np.uint32)
    same, other = [4000, 10, 997, 2500], [11, 2999]      # label 2 rows (r % 3 == 1), label 3 rows (r % 3 == 2)
    assert all(r % 3 == 1 for r in same) and all(r % 3 == 2 for r in other)
    v = rng.standard_normal(dim).astype(np.float32)
    raw[same + other] = v
    rq = np.stack([v, v, raw[7]])
    ql = np.array([2, 3, 2], np.uint32)
    for dtype, metric in (("f32", "cosine"), ("bf16", "l2"), ("bf16", "ip")):
        with va.Index(dim, dtype, metric) as ix:
            ix.add(raw)
            ix.set_labels(0, labels)
            ix.set_path(path)
            ids, sc = ix.search_labeled(rq, 6, ql)
        assert_same(ids, sc, *expected(O, raw, rq, ql, 6, dtype, metric, labels), f"{dtype}/{metric}")
        if metric != "ip":
            assert ids[0, :4].tolist() == sorted(same) and ids[1, :2].tolist() == sorted(other)
        assert not set(ids[0].tolist()) & set(other) and not set(ids[1].tolist()) & set(same)


# ---------------------------------------------------------------- k beyond a segment
@pytest.mark.parametrize("path", [PATH_GATHER, PATH_AUTO, PATH_STREAM])
def test_k_beyond_a_segment(va, O, world, path):
    labels, corpora, queries, _ = world
    raw, rq = corpora[64], queries[64][:6]
    ql = np.array([1, 63, 65, 1, L_NONE_A, 65], np.uint32)
    with va.Index(64, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_labels(0, labels)
        ix.set_path(path)
        ids, sc = ix.search_labeled(rq, 100, ql)
        assert_same(ids, sc, *expected(O, raw, rq, ql, 100, "bf16", "cosine", labels), "k=100")
        for q, rows in enumerate((1, 63, 65, 1, 0, 65)):
            assert (ids[q, :rows] != ID_NONE).all() and (ids[q, rows:] == ID_NONE).all() and np.isnan(sc[q, rows:]).all()
        ql2 = np.array([L_BIG, 64, L_BIG], np.uint32)
        ids, sc = ix.search_labeled(rq[:3], 3584, ql2)
        assert_same(ids, sc, *expected(O, raw, rq[:3], ql2, 3584, "bf16", "cosine", labels), "k=3584")
        assert (ids[1, 64:] == ID_NONE).all() and (ids[0] != ID_NONE).all()


# ---------------------------------------------------------------- filter, delete, update, compact, id_offset
@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "l2")])
def test_composition(va, O, world, dtype, metric):
    labels, corpora, queries, qlabels = world
    raw, rq, ql, k, off = corpora[64].copy(), queries[64][:300], qlabels[300], 10, 1_000_000
    rng = np.random.default_rng(9)
    allow = rng.random(N) < 0.7
    dead = np.concatenate([rng.choice(N, 3000, replace=False), np.flatnonzero(labels == 63)[:20], np.flatnonzero(labels == 1),
                           np.flatnonzero(labels == SMALL0 + 3)[:5]])
    dead = np.unique(dead)
    with va.Index(64, dtype, metric) as ix:
        ix.add(raw)
        ix.set_id_offset(off)
        ix.set_labels(off, labels[:N // 2])
        ix.set_labels(off + N // 2, labels[N // 2:])
        assert np.array_equal(ix.get_labels(off + 100, 1000), labels[100:1100])
        with pytest.raises(va.VrodError) as e:
            ix.set_labels(off - 1, labels[:4])
        assert e.value.code == 1
        ix.set_filter(allow)
        ix.delete(dead + off)
        ok = allow.copy()
        ok[dead] = False
        for path in (PATH_AUTO, PATH_GATHER, PATH_EXACT):
            ix.set_path(path)
            ids, sc = ix.search_labeled(rq, k, ql)
            assert_same(ids, sc, *expected(O, raw, rq, ql, k, dtype, metric, labels, ok, off), f"filter+delete path{path}")
        # update keeps the labels
        live = np.setdiff1d(np.arange(N), dead)
        upd = rng.choice(live, 500, replace=False)
        raw[upd] = rng.standard_normal((500, 64)).astype(np.float32)
        ix.update(upd + off, raw[upd])
        assert np.array_equal(ix.get_labels(off, N), labels)
        ix.set_path(PATH_AUTO)
        ids, sc = ix.search_labeled(rq, k, ql)
        assert_same(ids, sc, *expected(O, raw, rq, ql, k, dtype, metric, labels, ok, off), "after update")
        # compact moves the labels with their rows
        ix.compact()
        raw2, lab2, ok2 = raw[live], labels[live], allow[live]
        assert ix.count == live.size
        assert np.array_equal(ix.get_labels(off, live.size), lab2)
        for path in (PATH_AUTO, PATH_GATHER):
            ix.set_path(path)
            ids, sc = ix.search_labeled(rq, k, ql)
            assert_same(ids, sc, *expected(O, raw2, rq, ql, k, dtype, metric, lab2, ok2, off), f"after compact path{path}")
        # rows added later carry label 0
        extra = rng.standard_normal((700, 64)).astype(np.float32)
        ix.set_filter(None)
        ix.add(extra)
        lab3 = np.concatenate([lab2, np.zeros(700, np.uint32)])
        assert np.array_equal(ix.get_labels(off, lab3.size), lab3)
        ids, sc = ix.search_labeled(rq[:9], k, np.zeros(9, np.uint32))
        assert_same(ids, sc, *expected(O, np.concatenate([raw2, extra]), rq[:9], np.zeros(9, np.uint32), k, dtype, metric, lab3, None, off), "after add")


# ---------------------------------------------------------------- defaults and errors
def test_defaults_and_errors(va, O, world):
    import torch
    labels, corpora, queries, _ = world
    raw, rq, k = corpora[64][:20_000], queries[64][:40], 10
    with va.Index(64, "bf16", "cosine") as ix:
        ix.add(raw)
        ref = ix.search(rq, k)
        ids, sc = ix.search_labeled(rq, k, np.zeros(40, np.uint32))       # labels never set: every row is label 0
        assert_same(ids, sc, *ref, "unset labels, label 0")
        ids, sc = ix.search_labeled(rq, k, np.full(40, 7, np.uint32))
        assert (ids == ID_NONE).all() and np.isnan(sc).all()
        assert not ix.get_labels(0, 20_000).any()
        lab = labels[:20_000]
        ix.set_labels(0, lab)
        for first, n in ((19_999, 2), (20_000, 1), (1 << 40, 1)):           # not wholly within the rows: nothing changes
            with pytest.raises(va.VrodError) as e:
                ix.set_labels(first, np.full(n, 9, np.uint32))
            assert e.value.code == 1
        ix.set_labels(20_000, np.zeros(0, np.uint32))                       # n == 0 does nothing
        assert np.array_equal(ix.get_labels(0, 20_000), lab)
        with pytest.raises(va.VrodError) as e:
            ix.search_labeled(rq, 3585, np.zeros(40, np.uint32))
        assert e.value.code == 1
        bad = rq.copy()
        bad[3, 5] = np.nan
        with pytest.raises(va.VrodError) as e:
            ix.search_labeled(bad, k, np.zeros(40, np.uint32))
        assert e.value.code == 2
        ql = np.array([L_HALF, L_TENTH] * 20, np.uint32)
        want = expected(O, raw, rq, ql, k, "bf16", "cosine", lab)
        assert_same(*ix.search_labeled(rq, k, ql), *want, "after a rejected call")
        # a pending search blocks labels and labelled searches; after search_end both work
        dq = torch.from_numpy(rq).cuda()
        oi = torch.empty((40, k), dtype=torch.int64, device="cuda")
        osc = torch.empty((40, k), dtype=torch.float32, device="cuda")
        ix.search_begin_device(dq, k, oi, osc)
        for call in (lambda: ix.search_labeled(rq, k, ql), lambda: ix.set_labels(0, lab[:10]),
                     lambda: ix.search_labeled_device(dq, k, torch.from_numpy(ql.view(np.int32)).cuda())):
            with pytest.raises(va.VrodError) as e:
                call()
            assert e.value.code == 1
        ix.search_end()
        assert_same(*ix.search_labeled(rq, k, ql), *want, "after search_end")
    with va.Index(64, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        with pytest.raises(va.VrodError) as e:
            ix.set_labels(0, lab)
        assert e.value.code == 6
        with pytest.raises(va.VrodError) as e:
            ix.search_labeled(rq, k, np.zeros(40, np.uint32))
        assert e.value.code == 6
        assert not ix.get_labels(0, 100).any()


# ---------------------------------------------------------------- bystanders
def test_other_searches_ignore_labels(va, world):
    import torch
    labels, corpora, queries, qlabels = world
    raw, rq, k = corpora[100], queries[100][:300], 10
    with va.Index(100, "f32", "l2") as ix:
        ix.add(raw)
        dq = torch.from_numpy(rq).cuda()

        def everything():
            out = [ix.search(rq, k), ix.search(rq[:3], k)]
            out.append(ix.range_search(rq[:20], 150.0))
            bufs = [(torch.empty((300, k), dtype=torch.int64, device="cuda"), torch.empty((300, k), dtype=torch.float32, device="cuda")) for _ in range(2)]
            ix.search_begin_device(dq, k, *bufs[0])
            ix.search_begin_device(dq, k, *bufs[1])
            ix.search_end()
            ix.search_end()
            out += [(a.cpu().numpy().view(np.uint64), b.cpu().numpy()) for a, b in bufs]
            return out, ix.last_stats()
        before, st0 = everything()
        ix.set_labels(0, labels)
        ix.search_labeled(rq, k, qlabels[300])
        after, st1 = everything()
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        assert st0["scan_launches"] == st1["scan_launches"] and st0["path"] == st1["path"]


# ---------------------------------------------------------------- device form
def test_device_form_equals_host_form(va, world):
    import torch
    labels, corpora, queries, qlabels = world
    raw, rq, ql, k = corpora[100], queries[100], qlabels[300], 10
    with va.Index(100, "bf16", "ip") as ix:
        ix.add(raw)
        ix.set_labels(0, labels)
        hi, hs = ix.search_labeled(rq, k, ql)
        di, ds = ix.search_labeled_device(torch.from_numpy(rq).cuda(), k, torch.from_numpy(ql.view(np.int32)).cuda())
        assert_same(di.cpu().numpy().view(np.uint64), ds.cpu().numpy(), hi, hs, "device form")
