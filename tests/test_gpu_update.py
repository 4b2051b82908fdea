"""GPU tests of the in-place row update (vrod_index_update) against the CPU oracle.

The contract (DESIGN.md rule 11): after update(ids, rows) every search gives, bit for bit, what it gives on a fresh
handle built from raw' -- the rows given to add() with raw'[ids[i] - offset] = rows[i] applied in order -- so the
reference is the oracle over prepare(raw'), with deletions and a filter applied as rules 8 and 9 say.  Wherever the
certificate's bound is finite and the path is not EXACT, the observed |fast - canonical| must lie inside it.
"""
import numpy as np
import pytest

from support import (  # noqa: F401
    DT, METRIC_COSINE, METRIC_L2, PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, THREADS, va, bits, assert_same, check_bound, prep_of, form_of, eligible_rows, oracle_over)

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "ip"]


def oracle_live(O, raw, rq, k, dtype, metric, deleted=(), id_offset=0, allowed=None):
    """The oracle over the eligible rows of `raw` (not deleted, and allowed if a bool mask is given), ids mapped back."""
    return oracle_over(O, raw, rq, k, dtype, metric, eligible_rows(raw.shape[0], allowed, deleted), id_offset)


def applied(raw, ids, rows, offset=0):
    """raw' of the contract: the updates applied in order (the last occurrence of an id wins)."""
    out = raw.copy()
    for i, r in zip(np.asarray(ids, dtype=np.int64) - offset, rows):
        out[i] = r
    return out


# ---------------------------------------------------------------- every path x dtype x metric, 10 % updated, staged corpus
N_BIG, D_BIG = 300_000, 64


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(2025)
    raw = rng.standard_normal((N_BIG, D_BIG)).astype(np.float32)
    upd = np.sort(rng.choice(N_BIG, N_BIG // 10, replace=False))
    queries = rng.standard_normal((1024, D_BIG)).astype(np.float32)
    return raw, upd, queries


CASES = [  # (dtype, nq, path, VROD_F32_SPLIT, the path the stats must report, split_pass): test_gpu_delete.py CASES
    ("f32", 3, PATH_STREAM, None, PATH_STREAM, 0),
    ("bf16", 3, PATH_STREAM, None, PATH_STREAM, 0),
    ("bf16", 40, PATH_MFMA, None, PATH_MFMA, 0),        # skinny
    ("bf16", 300, PATH_MFMA, None, PATH_MFMA, 0),       # 4-wave
    ("bf16", 1024, PATH_MFMA, None, PATH_MFMA, 0),
    ("f32", 300, PATH_MFMA, "0", PATH_MFMA, 0),         # fp32 phased
    ("f32", 300, PATH_MFMA, "1", PATH_MFMA, 1),         # bf16 split planes
    ("f32", 5, PATH_EXACT, None, PATH_EXACT, 0),
    ("bf16", 5, PATH_EXACT, None, PATH_EXACT, 0),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype,nq,path,split,want_path,want_split", CASES)
def test_every_path_sees_the_update(va, oracle, big, metric, dtype, nq, path, split, want_path, want_split):
    """10 % of the rows updated, each query's current best two among them (they get random vectors and drop out) and
    the first updated rows turned into near copies of the queries (they come in).  The search BEFORE the update builds
    the bf16 planes of the split case, so what the later split pass reads of the updated rows is the scatter's write."""
    from conftest import f32_split
    raw, upd0, queries = big
    rq = queries[:nq]
    what = f"{metric}/{dtype}/nq={nq}/path={path}/split={split}"
    rng = np.random.default_rng(nq)
    with f32_split(split), va.Index(D_BIG, dtype, metric) as ix:
        ix.add(raw)
        ix.set_path(path)
        ids0, _ = ix.search(rq, 10)
        st0 = ix.last_stats()
        upd = np.unique(np.concatenate([upd0, ids0[:, :2].reshape(-1).astype(np.int64)]))
        rows = rng.standard_normal((upd.size, D_BIG)).astype(np.float32)
        m = min(nq, 64)
        rows[:m] = (1.0 if metric == "l2" else 2.0) * rq[:m] + 0.01 * rows[:m]     # (L2: next to the query itself)
        ix.update(upd, rows)
        assert ix.count == N_BIG and ix.live_count() == N_BIG and ix.filter_count() == N_BIG
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
        probe = np.concatenate([upd[:3], upd[-3:], [0, N_BIG - 1]])
        got = np.stack([ix.get_rows(int(r), 1)[0] for r in probe])
    raw2 = applied(raw, upd, rows)
    oi, osc = oracle_live(oracle, raw2, rq, 10, dtype, metric)
    assert_same(ids, sc, oi, osc, what)
    check_bound(st, what)
    assert st["path"] == want_path and st["split_pass"] == want_split and st0["split_pass"] == want_split, what
    assert np.isin(upd[:m].astype(np.uint64), ids).any(), f"{what}: no updated row among the results"
    assert np.array_equal(bits(got), bits(oracle.prepare(raw2[probe], DT[dtype], prep_of(metric)))), f"{what}: get_rows"
    if path == PATH_MFMA:
        assert st["scan_launches"] >= 3, f"{what}: not staged: {st}"


@pytest.mark.parametrize("dtype,nq,split", [("bf16", 300, None), ("bf16", 40, None), ("f32", 300, "1")])
def test_update_into_a_group_of_copies(va, oracle, big, dtype, nq, split):
    """Groups of 63 exact copies of a row; an update makes one more row -- with the smallest id of its group -- the
    64th copy.  The query is the group's row: the 10 best are the group's 10 smallest ids, the updated row first.  More
    equal candidates than k', so no certificate passes: the band pass has to resolve them."""
    from conftest import f32_split
    raw, _, _ = big
    raw = raw.copy()
    rng = np.random.default_rng(6)
    pos = np.sort(rng.choice(N_BIG, nq * 64, replace=False).reshape(nq, 64), axis=1)
    for g in range(nq):
        raw[pos[g, 1:]] = raw[pos[g, 1]]
    rq = np.ascontiguousarray(raw[pos[:, 1]])
    what = f"copies/{dtype}/nq={nq}/split={split}"
    with f32_split(split), va.Index(D_BIG, dtype, "cosine") as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        ix.search(rq, 10)                             # (builds the planes of the split case)
        ix.update(pos[:, 0], rq)
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
    raw2 = applied(raw, pos[:, 0], rq)
    oi, osc = oracle_live(oracle, raw2, rq, 10, dtype, "cosine")
    assert_same(ids, sc, oi, osc, what)
    assert np.array_equal(ids, pos[:, :10].astype(np.uint64)), what
    assert st["band_queries"] > 0, f"{what}: {st}"


# ---------------------------------------------------------------- edges
N_SMALL, D_SMALL = 40_000, 48


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(98)
    return rng.standard_normal((N_SMALL, D_SMALL)).astype(np.float32), rng.standard_normal((300, D_SMALL)).astype(np.float32)


@pytest.mark.parametrize("dtype,nq,path", [("bf16", 3, PATH_STREAM), ("f32", 300, PATH_MFMA), ("f32", 5, PATH_EXACT)])
def test_duplicates_errors_and_deletions(va, oracle, small, dtype, nq, path):
    raw, queries = small
    rq = queries[:nq]
    k = 8
    rng = np.random.default_rng(4)
    with va.Index(D_SMALL, dtype, "l2") as ix:
        ix.add(raw)
        ix.set_path(path)
        ix.update([], np.zeros((0, D_SMALL), np.float32))             # n == 0: nothing
        # an id named three times in one call: the last vector wins
        ids_u = np.array([5, 700, 5, 9, 5], dtype=np.int64)
        rows_u = np.stack([rq[0] * 1.01, rq[1] * 1.01, rq[0] * 1.02, rq[2 % nq] * 1.01, rq[0] * 1.001]).astype(np.float32)
        ix.update(ids_u, rows_u)
        cur = applied(raw, ids_u, rows_u)
        ids, sc = ix.search(rq, k)
        oi, osc = oracle_live(oracle, cur, rq, k, dtype, "l2")
        assert_same(ids, sc, oi, osc, "duplicates")
        assert ids[0, 0] == 5
        assert np.array_equal(bits(ix.get_rows(5, 1)), bits(oracle.prepare(rows_u[4:5], DT[dtype], METRIC_L2)))
        # update then delete: the row is gone; delete then update of that id: INVALID_ARG, nothing changes
        ix.delete([5, 12])
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
        oi, osc = oracle_live(oracle, cur, rq, k, dtype, "l2", [5, 12])
        assert_same(ids, sc, oi, osc, "update then delete")
        good = rng.standard_normal((3, D_SMALL)).astype(np.float32)
        for bad in ([7, 12, 8], [N_SMALL, 1, 2], [1, 2, 2**63], [3, 4, 5]):
            with pytest.raises(va.VrodError) as e:
                ix.update(bad, good)
            assert e.value.code == 1, bad
        # a NaN / Inf row in the middle of a batch: INVALID_VALUE, nothing changes -- not even the bound
        for poison in (np.nan, np.inf):
            rows_bad = (rng.standard_normal((5, D_SMALL)) * 100).astype(np.float32)   # large norms: a written max would show
            rows_bad[2, 17] = poison
            with pytest.raises(va.VrodError) as e:
                ix.update([20, 21, 22, 23, 24], rows_bad)
            assert e.value.code == 2
        ids2, sc2 = ix.search(rq, k)
        st2 = ix.last_stats()
        assert np.array_equal(ids2, ids) and np.array_equal(bits(sc2), bits(sc))
        assert bits(np.float32(st2["eps_bound"])) == bits(np.float32(st["eps_bound"])), (st, st2)
        assert np.array_equal(bits(ix.get_rows(20, 5)), bits(oracle.prepare(cur[20:25], DT[dtype], METRIC_L2)))
        assert ix.count == N_SMALL and ix.live_count() == N_SMALL - 2
        # a valid update still applies afterwards, beside the deletions
        ix.update([7, 8, 13], good)
        cur = applied(cur, [7, 8, 13], good)
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
        oi, osc = oracle_live(oracle, cur, rq, k, dtype, "l2", [5, 12])
        assert_same(ids, sc, oi, osc, "update beside deletions")
        check_bound(st, "update beside deletions")


def test_update_larger_than_one_staging_chunk(va, oracle, small):
    """More rows than one staged chunk (65536): the call checks every row first, then writes; a NaN in the LAST chunk
    leaves the first chunk's rows untouched."""
    raw, queries = small
    rng = np.random.default_rng(14)
    n, dim = 150_000, 16
    base = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((4, dim)).astype(np.float32)
    order = rng.permutation(n)[:100_000]
    rows = rng.standard_normal((order.size, dim)).astype(np.float32)
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add(base)
        bad = rows.copy()
        bad[-1, 3] = np.nan
        with pytest.raises(va.VrodError) as e:
            ix.update(order, bad)
        assert e.value.code == 2
        assert np.array_equal(bits(ix.get_rows(0, n)), bits(oracle.prepare(base, 1, METRIC_COSINE, threads=THREADS)))
        ix.update(order, rows)
        cur = applied(base, order, rows)
        assert np.array_equal(bits(ix.get_rows(0, n)), bits(oracle.prepare(cur, 1, METRIC_COSINE, threads=THREADS)))
        ids, sc = ix.search(rq, 10)
    oi, osc = oracle_live(oracle, cur, rq, 10, "bf16", "cosine")
    assert_same(ids, sc, oi, osc, "two chunks")


@pytest.mark.parametrize("nq,path", [(3, PATH_STREAM), (300, PATH_MFMA), (3, PATH_EXACT)])
def test_id_offset(va, oracle, small, nq, path):
    raw, queries = small
    off = 1_000_000
    rq = queries[:nq]
    rng = np.random.default_rng(nq)
    with va.Index(D_SMALL, "bf16", "ip") as ix:
        ix.set_id_offset(off)
        ix.add(raw)
        ix.set_path(path)
        upd = np.sort(rng.choice(N_SMALL, 4000, replace=False))
        rows = (3.0 * rng.standard_normal((upd.size, D_SMALL))).astype(np.float32)
        for bad in ([0], [off - 1], [off + N_SMALL]):
            with pytest.raises(va.VrodError) as e:
                ix.update(bad, rows[:1])
            assert e.value.code == 1
        ix.update(upd + off, rows)
        ids, sc = ix.search(rq, 10)
    oi, osc = oracle_live(oracle, applied(raw, upd, rows), rq, 10, "bf16", "ip", id_offset=off)
    assert_same(ids, sc, oi, osc, f"offset/nq={nq}/path={path}")
    assert np.isin(ids, (upd + off).astype(np.uint64)).any()


@pytest.mark.parametrize("dtype,nq,path,frac", [("bf16", 300, PATH_AUTO, 0.5), ("f32", 3, PATH_AUTO, 0.5), ("bf16", 300, PATH_AUTO, 0.001),
                                                ("f32", 40, PATH_GATHER, 0.3)])
def test_update_under_a_filter(va, oracle, small, dtype, nq, path, frac):
    """A filter and deletions in place: allowed and not-allowed rows are updated alike; the filter, the tombstones
    and the three counts stay as they were."""
    raw, queries = small
    rq = queries[:nq]
    rng = np.random.default_rng(31)
    allow = rng.random(N_SMALL - 1000) < frac
    deleted = np.sort(rng.choice(N_SMALL, 2000, replace=False))
    with va.Index(D_SMALL, dtype, "cosine") as ix:
        ix.add(raw)
        ix.delete(deleted)
        ix.set_filter(allow)
        ix.set_path(path)
        fc = ix.filter_count()
        ids0, _ = ix.search(rq, 10)
        hits = ids0[ids0 != ID_NONE].astype(np.int64)
        upd = np.setdiff1d(np.unique(np.concatenate([hits[:50], rng.choice(N_SMALL, 4000, replace=False)])), deleted)
        rows = rng.standard_normal((upd.size, D_SMALL)).astype(np.float32)
        m = min(nq, 20)
        rows[-m:] = rq[:m] + 0.01 * rows[-m:]
        ix.update(upd, rows)
        assert ix.filter_count() == fc and ix.live_count() == N_SMALL - deleted.size and ix.count == N_SMALL
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
    oi, osc = oracle_live(oracle, applied(raw, upd, rows), rq, 10, dtype, "cosine", deleted, allowed=allow)
    assert_same(ids, sc, oi, osc, f"filter/{dtype}/nq={nq}/{frac}")
    check_bound(st, "filter")
    if path == PATH_GATHER:
        assert st["path"] == PATH_GATHER, st


@pytest.mark.parametrize("dtype,metric,nq", [("bf16", "cosine", 300), ("f32", "l2", 40), ("f32", "ip", 3)])
def test_range_search_after_an_update(va, oracle, small, dtype, metric, nq):
    raw, queries = small
    rq = queries[:nq]
    rng = np.random.default_rng(41)
    upd = np.sort(rng.choice(N_SMALL, 4000, replace=False))
    rows = rng.standard_normal((upd.size, D_SMALL)).astype(np.float32)
    m = min(nq, 30)
    rows[:m] = rq[:m] + 0.05 * rows[:m]
    deleted = np.arange(3, N_SMALL, 50)
    upd = np.setdiff1d(upd, deleted)
    rows = rows[:upd.size]
    raw2 = applied(raw, upd, rows)
    mask = np.ones(N_SMALL, bool)
    mask[deleted] = False
    # thresholds that keep a few dozen rows per query: the 30th best score of the reference
    pc = oracle.prepare(raw2, DT[dtype], prep_of(metric), threads=THREADS)
    pq = oracle.prepare(rq, DT[dtype], prep_of(metric), threads=THREADS)
    _, s30 = oracle.scan_topk(pc[mask], pq, 30, form_of(metric), threads=THREADS)
    thr = s30[:, -1].copy()
    olims, oids, osc = oracle.scan_range(pc, pq, thr, form_of(metric), mask=mask, threads=THREADS)
    with va.Index(D_SMALL, dtype, metric) as ix:
        ix.add(raw)
        ix.delete(deleted)
        ix.range_search(rq, thr)
        ix.update(upd, rows)
        lims, ids, sc = ix.range_search(rq, thr)
    assert np.array_equal(lims, olims), f"range/{dtype}/{metric}"
    assert np.array_equal(ids, oids) and np.array_equal(bits(sc), bits(osc)), f"range/{dtype}/{metric}"
    assert int(lims[-1]) >= 30 * nq


# ---------------------------------------------------------------- pipelined form and graph replay
def test_update_while_pending_fails_then_applies(va, oracle, small):
    import torch
    raw, queries = small
    dev = torch.device("cuda", 0)
    nq, k = 300, 10
    q = torch.from_numpy(np.ascontiguousarray(queries[:nq])).to(dev)
    outs = [(torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev)) for _ in range(2)]
    with va.Index(D_SMALL, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.search_begin_device(q, k, *outs[0])
        with pytest.raises(va.VrodError) as e:
            ix.update([0], raw[:1])
        assert e.value.code == 1
        ix.search_end()
        top = np.unique(outs[0][0].cpu().numpy().view(np.uint64)[:, 0]).astype(np.int64)
        rows = np.ascontiguousarray(-raw[top])               # the best row becomes the worst
        ix.update(top, rows)
        ix.search_begin_device(q, k, *outs[1])
        ix.search_end()
        torch.cuda.synchronize()
        ids, sc = outs[1][0].cpu().numpy().view(np.uint64), outs[1][1].cpu().numpy()
    oi, osc = oracle_live(oracle, applied(raw, top, rows), queries[:nq], k, "bf16", "cosine")
    assert_same(ids, sc, oi, osc, "pipelined")


def test_graph_replay_sees_the_update(va, oracle):
    """The pipeline of test_gpu_delete.py::test_graph_replay_sees_the_delete with an update between the two runs: an
    update changes no pointer and no size, so the captured graphs stay valid -- and every replayed step must read the
    new rows."""
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

    with va.Index(dim, "f32", "cosine") as ix:
        ix.add(raw)
        before = pipeline(ix, 10)                     # each slot: plain, capture, then replays
        oi, osc = oracle_live(oracle, raw, rq, k, "f32", "cosine")
        for ids, sc in before:
            assert_same(ids, sc, oi, osc, "before")
        # the best row of query 0 turns away, row 4321 becomes query 1 itself
        upd = [int(before[-1][0][0, 0]), 4321]
        rows = np.stack([-raw[upd[0]], rq[1]]).astype(np.float32)
        ix.update(upd, rows)
        cur = applied(raw, upd, rows)
        after = pipeline(ix, 10)
        oi, osc = oracle_live(oracle, cur, rq, k, "f32", "cosine")
        for step, (ids, sc) in enumerate(after):
            assert ids[1, 0] == 4321 and upd[0] not in ids[0], f"step {step}"
            assert_same(ids, sc, oi, osc, f"after, step {step}")
        ix.update([int(after[-1][0][0, 0])], rq[:1] * 0.5)
        cur = applied(cur, [int(after[-1][0][0, 0])], rq[:1] * 0.5)
        again = pipeline(ix, 8)
        oi, osc = oracle_live(oracle, cur, rq, k, "f32", "cosine")
        for step, (ids, sc) in enumerate(again):
            assert_same(ids, sc, oi, osc, f"second update, step {step}")


# ---------------------------------------------------------------- multi-device handle
@pytest.mark.parametrize("metric,nq,path", [("cosine", 3, PATH_STREAM), ("l2", 300, PATH_MFMA), ("ip", 3, PATH_EXACT)])
def test_multi_device_routes_updates_to_shards(va, oracle, metric, nq, path):
    rng = np.random.default_rng(22)
    n, dim, k = 200_000, 32, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((nq, dim)).astype(np.float32)
    # both sides of the 65536-row block boundaries (shard 0 | shard 1 | shard 0 ...), and random rows
    upd = np.unique(np.concatenate([np.arange(65530, 65542), np.arange(131068, 131076), rng.choice(n, 5000, replace=False)]))
    with va.Index(dim, "f32", metric, devices=[0, 0]) as ix:
        ix.add(raw)
        ix.set_path(path)
        ids0, _ = ix.search(rq, k)
        upd = np.unique(np.concatenate([upd, ids0[:, :2].reshape(-1).astype(np.int64)]))
        upd = upd[upd != 70000]                                       # (deleted below)
        rows = rng.standard_normal((upd.size, dim)).astype(np.float32)
        b = np.searchsorted(upd, [65535, 65536, 131071, 131072])      # rows at the boundaries become the queries' best
        rows[b] = 2.0 * rq[np.arange(4) % nq]
        # all or nothing over the handle as a whole: a bad id, a deleted row, a NaN on the second shard
        ix.delete([70000])
        for bad_ids, bad_rows, code in (([1, n], rows[:2], 1), ([1, 70000], rows[:2], 1),
                                        ([1, 65536], np.stack([rows[0], np.full(dim, np.nan, np.float32)]), 2)):
            with pytest.raises(va.VrodError) as e:
                ix.update(bad_ids, bad_rows)
            assert e.value.code == code
        assert np.array_equal(bits(ix.get_rows(1, 1)), bits(oracle.prepare(raw[1:2], 0, prep_of(metric))))
        ix.update(upd, rows)
        assert ix.count == n and ix.live_count() == n - 1
        ids, sc = ix.search(rq, k)
        edge = ix.get_rows(65530, 12)
    raw2 = applied(raw, upd, rows)
    oi, osc = oracle_live(oracle, raw2, rq, k, "f32", metric, [70000])
    assert_same(ids, sc, oi, osc, f"multi/{metric}/nq={nq}/path={path}")
    assert np.array_equal(bits(edge), bits(oracle.prepare(raw2[65530:65542], 0, prep_of(metric))))
