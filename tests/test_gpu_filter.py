"""GPU tests of the allow-list filter (vrod_index_set_filter) against the CPU oracle over the eligible rows.

The contract: a search on a handle with a filter returns, bit for bit, what the oracle returns over the eligible rows
only -- eligible = sorted(allowed & live) -- with the ids mapped back: scan_topk(prepared[eligible], ...), then every id
i != ID_NONE becomes eligible[i].  eligible is increasing, so ties still break by the smaller id, and slots beyond the
eligible rows are (ID_NONE, NaN).  Wherever the path is not EXACT or GATHER, the observed |fast - canonical| must lie
inside the certificate's bound; a GATHER search reports no fast pass at all.
"""
import numpy as np
import pytest

from support import (  # noqa: F401
    PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, va, assert_same, eligible_rows, oracle_over, row_bytes)

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "ip"]


def check_stats(st, what, m=None, row_bytes=None, dim=None):
    if st["path"] == PATH_GATHER:
        assert st["fallback_queries"] == 0 and st["band_queries"] == 0, f"{what}: {st}"
        assert st["max_fast_err"] == 0 and st["eps_bound"] == 0, f"{what}: {st}"
        if m is not None and m > 0:
            assert st["scan_bytes"] == m * row_bytes, f"{what}: {st}"
            assert st["scan_flops"] == 2.0 * st["nq"] * m * dim, f"{what}: {st}"
    elif st["path"] != PATH_EXACT and np.isfinite(st["eps_bound"]):
        assert st["max_fast_err"] <= st["eps_bound"], f"{what}: {st}"


# ---------------------------------------------------------------- every path x dtype x metric x filter kind
N_BIG, D_BIG = 300_000, 64


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(4242)
    raw = rng.standard_normal((N_BIG, D_BIG)).astype(np.float32)
    queries = rng.standard_normal((1024, D_BIG)).astype(np.float32)
    single = np.zeros(N_BIG, bool)
    single[123_457] = True
    block = np.zeros(N_BIG, bool)
    block[200_000:203_000] = True
    filters = {
        "half": rng.random(N_BIG) < 0.5,
        "one_pct": rng.random(N_BIG) < 0.01,
        "block": block,
        "single": single,
        "empty": np.zeros(N_BIG, bool),
    }
    return raw, queries, filters


PATHS = [  # (forced path, nq)
    (PATH_STREAM, 3), (PATH_MFMA, 300), (PATH_MFMA, 1024), (PATH_EXACT, 5), (PATH_GATHER, 1024), (PATH_GATHER, 3),
    (PATH_AUTO, 1024), (PATH_AUTO, 3),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_path_honours_the_filter(va, oracle, big, metric, dtype):
    raw, queries, filters = big
    k = 10
    with va.Index(D_BIG, dtype, metric) as ix:
        ix.add(raw)
        assert ix.filter_count() == N_BIG
        for kind, allow in filters.items():
            ix.set_filter(allow)
            el = eligible_rows(N_BIG, allow)
            assert ix.filter_count() == el.size and ix.live_count() == N_BIG and ix.count == N_BIG
            oi, osc = oracle_over(oracle, raw, queries, k, dtype, metric, el)
            for path, nq in PATHS:
                what = f"{metric}/{dtype}/{kind}/path={path}/nq={nq}"
                ix.set_path(path)
                ids, sc = ix.search(queries[:nq], k)
                st = ix.last_stats()
                assert_same(ids, sc, oi[:nq], osc[:nq], what)
                check_stats(st, what, el.size, row_bytes(dtype, D_BIG), D_BIG)
                if path != PATH_AUTO:
                    assert st["path"] == path, f"{what}: {st}"
                if el.size < k:
                    assert (ids[:, el.size:] == ID_NONE).all() and np.isnan(sc[:, el.size:]).all(), what
            ix.set_path(PATH_AUTO)


def test_auto_gathers_a_narrow_filter_and_scans_a_broad_one(va, oracle, big):
    raw, queries, filters = big
    with va.Index(D_BIG, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_filter(filters["single"])
        ix.search(queries, 10)
        assert ix.last_stats()["path"] == PATH_GATHER
        ix.set_filter(filters["half"])
        ix.search(queries, 10)
        assert ix.last_stats()["path"] == PATH_MFMA
        ix.set_filter(None)
        ix.search(queries, 10)
        assert ix.last_stats()["path"] == PATH_MFMA


@pytest.mark.parametrize("split", ["1", "0"])
def test_fp32_mfma_forms_under_a_filter(va, oracle, big, split):
    from conftest import f32_split
    raw, queries, filters = big
    nq, k = 300, 10
    with f32_split(split), va.Index(D_BIG, "f32", "cosine") as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        for kind in ("half", "one_pct"):
            ix.set_filter(filters[kind])
            ids, sc = ix.search(queries[:nq], k)
            st = ix.last_stats()
            assert st["split_pass"] == (1 if split == "1" else 0), st
            oi, osc = oracle_over(oracle, raw, queries[:nq], k, "f32", "cosine", eligible_rows(N_BIG, filters[kind]))
            assert_same(ids, sc, oi, osc, f"split={split}/{kind}")
            check_stats(st, f"split={split}/{kind}")


def test_band_pass_with_copies_under_a_filter(va, oracle, big):
    """Groups of 64 exact copies of a row; the filter allows 40 of each group, not the query's own row.  The 10 best are
    the 10 smallest allowed ids of the group: more equal candidates than k', so the band pass resolves them."""
    raw, _, _ = big
    raw = raw.copy()
    nq = 300
    rng = np.random.default_rng(6)
    pos = rng.choice(N_BIG, nq * 64, replace=False).reshape(nq, 64)
    for g in range(nq):
        raw[pos[g]] = raw[pos[g, 0]]
    rq = np.ascontiguousarray(raw[pos[:, 0]])
    allow = rng.random(N_BIG) < 0.5
    allow[pos[:, 0]] = False
    for g in range(nq):
        allow[pos[g, 1:]] = False
        allow[pos[g, 1 + rng.permutation(63)[:40]]] = True
    with va.Index(D_BIG, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        ix.set_filter(allow)
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
    oi, osc = oracle_over(oracle, raw, rq, 10, "bf16", "cosine", eligible_rows(N_BIG, allow))
    assert_same(ids, sc, oi, osc, "copies")
    for g in range(nq):
        allowed = np.sort(pos[g][allow[pos[g]]])
        assert np.array_equal(ids[g], allowed[:10].astype(np.uint64))
    assert st["band_queries"] > 0, st
    check_stats(st, "copies")


# ---------------------------------------------------------------- semantics: short filters, adds, deletes, clearing
N_SMALL, D_SMALL = 40_000, 48
SMALL_PATHS = [(PATH_STREAM, 3), (PATH_MFMA, 300), (PATH_EXACT, 5), (PATH_GATHER, 300), (PATH_AUTO, 300), (PATH_AUTO, 3)]


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(98)
    return rng.standard_normal((N_SMALL, D_SMALL)).astype(np.float32), rng.standard_normal((300, D_SMALL)).astype(np.float32)


def run_paths(ix, O, raw, queries, k, dtype, metric, el, what, id_offset=0):
    oi, osc = oracle_over(O, raw, queries, k, dtype, metric, el, id_offset)
    for path, nq in SMALL_PATHS:
        ix.set_path(path)
        ids, sc = ix.search(queries[:nq], k)
        assert_same(ids, sc, oi[:nq], osc[:nq], f"{what}/path={path}/nq={nq}")
        check_stats(ix.last_stats(), f"{what}/path={path}")
    ix.set_path(PATH_AUTO)


def test_short_filter_deletes_adds_and_clearing(va, oracle, small):
    raw, queries = small
    rng = np.random.default_rng(1)
    k, dtype, metric = 12, "f32", "l2"
    allow = rng.random(30_000) < 0.3                      # shorter than count: rows 30000.. are not allowed
    with va.Index(D_SMALL, dtype, metric) as ix:
        ix.add(raw)
        before = rng.choice(N_SMALL, 2000, replace=False)
        ix.delete(before)                                  # deletes before the filter
        ix.set_filter(allow)
        el = eligible_rows(N_SMALL, allow, before)
        assert ix.filter_count() == el.size and ix.live_count() == N_SMALL - 2000
        run_paths(ix, oracle, raw, queries, k, dtype, metric, el, "short")
        after = np.concatenate([el[:50], rng.choice(N_SMALL, 500, replace=False)])
        ix.delete(after)                                   # deletes after it are honoured
        deleted = np.union1d(before, after)
        el = eligible_rows(N_SMALL, allow, deleted)
        assert ix.filter_count() == el.size
        run_paths(ix, oracle, raw, queries, k, dtype, metric, el, "deleted after")
        more = np.ascontiguousarray(queries[:8] * 1.001)   # the queries' nearest rows, added after the filter: not allowed
        ix.add(more)
        full = np.concatenate([raw, more])
        assert ix.count == N_SMALL + 8 and ix.filter_count() == el.size
        run_paths(ix, oracle, full, queries, k, dtype, metric, el, "added after")
        with pytest.raises(va.VrodError) as e:           # longer than count: refused, nothing changes
            ix.set_filter(np.ones(N_SMALL + 9, bool))
        assert e.value.code == 1 and ix.filter_count() == el.size
        ix.set_filter(np.ones(N_SMALL + 8, bool))          # a filter that names the new rows
        el_all = eligible_rows(N_SMALL + 8, np.ones(N_SMALL + 8, bool), deleted)
        assert ix.filter_count() == el_all.size
        run_paths(ix, oracle, full, queries, k, dtype, metric, el_all, "refilter")
        ix.set_filter(None)                                # cleared: the unfiltered (delete-only) results
        assert ix.filter_count() == ix.live_count()
        run_paths(ix, oracle, full, queries, k, dtype, metric, el_all, "cleared")
        ix.set_filter(np.zeros(0, bool))                   # an empty allow-list: every slot unfilled
        assert ix.filter_count() == 0
        for path, nq in SMALL_PATHS:
            ix.set_path(path)
            ids, sc = ix.search(queries[:nq], k)
            assert (ids == ID_NONE).all() and np.isnan(sc).all(), f"empty/path={path}"


@pytest.mark.parametrize("metric", METRICS)
def test_id_offset(va, oracle, small, metric):
    raw, queries = small
    off = 5_000_000
    allow = np.zeros(N_SMALL, bool)
    allow[::97] = True
    with va.Index(D_SMALL, "bf16", metric) as ix:
        ix.set_id_offset(off)
        ix.add(raw)
        ix.set_filter(allow)
        ix.delete(np.array([97 * 3, 97 * 5]) + off)
        el = eligible_rows(N_SMALL, allow, [97 * 3, 97 * 5])
        run_paths(ix, oracle, raw, queries, 10, "bf16", metric, el, f"offset/{metric}", id_offset=off)


def test_k_beyond_the_eligible_rows(va, oracle, small):
    raw, queries = small
    allow = np.zeros(N_SMALL, bool)
    allow[[3, 77, 39_999]] = True
    with va.Index(D_SMALL, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_filter(allow)
        run_paths(ix, oracle, raw, queries, 100, "bf16", "cosine", np.array([3, 77, 39_999]), "k>m")


# ---------------------------------------------------------------- sample window under a 10 % filter at scale
def test_ten_percent_filter_keeps_the_certificates(va):
    """1M x 768 bf16, 10 % of the rows allowed (none of the first 300k), batch 1024: the dense MFMA path must find its
    first threshold on eligible rows (no failed certificate), and its results are the gather path's bits."""
    import torch
    n, dim, nq, k = 1_000_000, 768, 1024, 10
    rng = np.random.default_rng(8)
    allow = rng.random(n) < 0.1
    allow[:300_000] = False
    dev = torch.device("cuda", 0)
    out = [(torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)) for _ in range(2)]
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add_synthetic(11, 0, n)
        ix.set_filter(allow)
        ix.set_path(PATH_MFMA)
        ix.search_synthetic_device(12, 0, nq, k, *out[0])
        torch.cuda.synchronize()
        st = ix.last_stats()
        ix.set_path(PATH_GATHER)
        ix.search_synthetic_device(12, 0, nq, k, *out[1])
        torch.cuda.synchronize()
        sg = ix.last_stats()
    assert st["path"] == PATH_MFMA and st["fallback_queries"] == 0, st
    check_stats(st, "ten")
    assert sg["path"] == PATH_GATHER, sg
    a = [(o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy()) for o in out]
    assert_same(a[0][0], a[0][1], a[1][0], a[1][1], "ten: mfma vs gather")
    assert np.isin(a[0][0], np.flatnonzero(allow).astype(np.uint64)).all()


# ---------------------------------------------------------------- pipelined form and graph replay
def test_filter_while_pending_fails_then_applies(va, oracle, small):
    import torch
    raw, queries = small
    dev = torch.device("cuda", 0)
    nq, k = 300, 10
    q = torch.from_numpy(np.ascontiguousarray(queries[:nq])).to(dev)
    outs = [(torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)) for _ in range(3)]
    allow = np.zeros(N_SMALL, bool)
    allow[::50] = True
    with va.Index(D_SMALL, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.search_begin_device(q, k, *outs[0])
        with pytest.raises(va.VrodError) as e:
            ix.set_filter(allow)
        assert e.value.code == 1
        ix.search_end()
        assert ix.filter_count() == N_SMALL
        ix.set_filter(allow)
        got = []
        for path in (PATH_GATHER, PATH_MFMA):             # two filtered searches in flight on each path
            ix.set_path(path)
            ix.search_begin_device(q, k, *outs[1])
            ix.search_begin_device(q, k, *outs[2])
            ix.search_end()
            ix.search_end()
            torch.cuda.synchronize()
            got += [(o[0].cpu().numpy().view(np.uint64).copy(), o[1].cpu().numpy().copy()) for o in outs[1:]]
    oi, osc = oracle_over(oracle, raw, queries[:nq], k, "bf16", "cosine", np.flatnonzero(allow))
    for i, (ids, sc) in enumerate(got):
        assert_same(ids, sc, oi, osc, f"pipelined {i}")


def test_graph_replay_sees_every_filter_change(va, oracle):
    """Small stream-path searches begun while another is pending with the same buffers are captured and replayed.  The
    filter's device mask keeps its address when the filter changes: the replayed search must see the new contents."""
    import torch
    dev = torch.device("cuda", 0)
    n, dim, k, nq = 10000, 128, 10, 2
    raw = oracle.synth_rows(1, 0, n, dim)
    rq = oracle.synth_rows(2, 0, nq, dim)
    q = [torch.from_numpy(rq).to(dev) for _ in range(2)]
    o = [(torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)) for _ in range(2)]

    def pipeline(ix, steps):
        res = []
        ix.search_begin_device(q[0], k, *o[0])
        for s in range(1, steps):
            ix.search_begin_device(q[s % 2], k, *o[s % 2])
            ix.search_end()
            p = (s - 1) % 2
            res.append((o[p][0].cpu().numpy().view(np.uint64).copy(), o[p][1].cpu().numpy().copy()))
        ix.search_end()
        p = (steps - 1) % 2
        res.append((o[p][0].cpu().numpy().view(np.uint64).copy(), o[p][1].cpu().numpy().copy()))
        return res

    rng = np.random.default_rng(3)
    a, b = rng.random(n) < 0.5, rng.random(n) < 0.5
    with va.Index(dim, "f32", "cosine") as ix:
        ix.add(raw)
        ix.set_path(PATH_STREAM)
        gone = []
        for what in ("filter a", "filter b", "delete under b", "cleared"):
            if what == "filter a":
                ix.set_filter(a)
                allow = a
            elif what == "filter b":                      # same mask buffer, other contents
                ix.set_filter(b)
                allow = b
            elif what == "delete under b":
                gone = [int(r) for r in np.flatnonzero(b)[:2]]
                ix.delete(gone)
            else:
                ix.set_filter(None)
                allow = np.ones(n, bool)
            oi, osc = oracle_over(oracle, raw, rq, k, "f32", "cosine", eligible_rows(n, allow, gone))
            for step, (ids, sc) in enumerate(pipeline(ix, 8)):
                assert_same(ids, sc, oi, osc, f"{what}, step {step}")


# ---------------------------------------------------------------- multi-device handle (two shards on one device)
@pytest.mark.parametrize("metric,nq,path", [("cosine", 3, PATH_STREAM), ("l2", 300, PATH_MFMA), ("ip", 3, PATH_EXACT),
                                            ("cosine", 300, PATH_GATHER), ("l2", 300, PATH_AUTO)])
def test_multi_device_routes_the_filter_to_shards(va, oracle, metric, nq, path):
    rng = np.random.default_rng(22)
    n, dim, k = 200_000, 32, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((nq, dim)).astype(np.float32)
    allow = rng.random(190_007) < 0.05                # shorter than count, ends mid-block of shard 0
    allow[65530:65542] = True                         # both sides of a shard block boundary
    allow[131068:131076] = True
    with va.Index(dim, "f32", metric, devices=[0, 0]) as ix:
        ix.add(raw)
        ix.set_path(path)
        ix.set_filter(allow)
        deleted = np.array([65531, 131070, 7])
        ix.delete(deleted)
        el = eligible_rows(n, allow, deleted)
        assert ix.filter_count() == el.size
        ids, sc = ix.search(rq, k)
        oi, osc = oracle_over(oracle, raw, rq, k, "f32", metric, el)
        assert_same(ids, sc, oi, osc, f"multi/{metric}/nq={nq}/path={path}")
        ix.set_filter(None)
        assert ix.filter_count() == n - deleted.size
        ids, sc = ix.search(rq, k)
        oi, osc = oracle_over(oracle, raw, rq, k, "f32", metric, eligible_rows(n, np.ones(n, bool), deleted))
        assert_same(ids, sc, oi, osc, f"multi cleared/{metric}/nq={nq}/path={path}")
