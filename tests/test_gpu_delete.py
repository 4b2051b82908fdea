"""GPU tests of row deletion (vrod_index_delete) against the CPU oracle over the live rows.

The contract: a search over a handle with deleted rows returns, bit for bit, what the oracle returns over the live
rows only, with the ids mapped back -- live = sorted(set(range(N)) - deleted), scan_topk(prepared[live], ...), then
every id i != ID_NONE becomes live[i].  live is increasing, so ties still break by the smaller id, and slots beyond
the live rows are (ID_NONE, NaN).  Wherever the certificate's bound is finite and the path is not EXACT, the observed
|fast - canonical| must lie inside it.
"""
import numpy as np
import pytest

from support import (  # noqa: F401
    PATH_STREAM, PATH_MFMA, PATH_EXACT, ID_NONE, va, bits, assert_same, check_bound, eligible_rows, oracle_over)

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "ip"]


def oracle_live(O, raw, rq, k, dtype, metric, deleted, id_offset=0):
    """The oracle over the live rows of `raw`, ids mapped back (+ id_offset)."""
    return oracle_over(O, raw, rq, k, dtype, metric, eligible_rows(raw.shape[0], deleted=deleted), id_offset)


def search_case(va, O, raw, rq, k, dtype, metric, deleted, path, split=None, what=""):
    from conftest import f32_split
    with f32_split(split), va.Index(raw.shape[1], dtype, metric) as ix:
        ix.add(raw)
        ix.delete(deleted)
        ix.set_path(path)
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
        assert ix.live_count() == raw.shape[0] - np.unique(deleted).size
        assert ix.count == raw.shape[0]
    oi, osc = oracle_live(O, raw, rq, k, dtype, metric, deleted)
    assert_same(ids, sc, oi, osc, what)
    check_bound(st, what)
    return ids, sc, st


# ---------------------------------------------------------------- every path x dtype x metric, 10 % deleted, staged corpus
N_BIG, D_BIG = 300_000, 64


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(2024)
    raw = rng.standard_normal((N_BIG, D_BIG)).astype(np.float32)
    deleted = np.sort(rng.choice(N_BIG, N_BIG // 10, replace=False))
    queries = rng.standard_normal((1024, D_BIG)).astype(np.float32)
    return raw, deleted, queries


CASES = [  # (dtype, nq, path, VROD_F32_SPLIT, the path the stats must report, split_pass)
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
def test_every_path_honours_deletions(va, oracle, big, metric, dtype, nq, path, split, want_path, want_split):
    raw, deleted, queries = big
    what = f"{metric}/{dtype}/nq={nq}/path={path}/split={split}"
    _, _, st = search_case(va, oracle, raw, queries[:nq], 10, dtype, metric, deleted, path, split, what)
    assert st["path"] == want_path, what
    assert st["split_pass"] == want_split, what
    if path == PATH_MFMA:
        assert st["scan_launches"] >= 3, f"{what}: not staged: {st}"   # sample pass + filtered stages


# ---------------------------------------------------------------- the query's own row is deleted
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype,nq,path", [("bf16", 3, PATH_STREAM), ("bf16", 300, PATH_MFMA), ("f32", 40, PATH_MFMA),
                                           ("f32", 3, PATH_EXACT)])
def test_deleted_query_row_never_comes_back(va, oracle, big, metric, dtype, nq, path):
    raw, _, _ = big
    rng = np.random.default_rng(77)
    qrows = np.sort(rng.choice(N_BIG, nq, replace=False))
    rq = np.ascontiguousarray(raw[qrows])
    what = f"self/{metric}/{dtype}/nq={nq}/path={path}"
    ids, _, _ = search_case(va, oracle, raw, rq, 10, dtype, metric, qrows, path, None, what)
    assert not np.isin(ids, qrows.astype(np.uint64)).any(), what


@pytest.mark.parametrize("dtype,nq,split", [("bf16", 300, None), ("bf16", 40, None), ("f32", 300, "1")])
def test_surviving_copies_come_back_in_id_order(va, oracle, big, dtype, nq, split):
    """Groups of 64 exact copies of a row; the query is the group's row, 8 copies of each group are deleted (the
    query's own row among them).  The 10 best are the 10 smallest surviving ids of the group: more equal candidates
    than k' (18, 42 on the split pass), so no certificate passes -- the band pass has to resolve them."""
    raw, _, _ = big
    raw = raw.copy()
    rng = np.random.default_rng(5)
    pos = rng.choice(N_BIG, nq * 64, replace=False).reshape(nq, 64)
    for g in range(nq):
        raw[pos[g]] = raw[pos[g, 0]]
    rq = np.ascontiguousarray(raw[pos[:, 0]])
    deleted = np.concatenate([pos[:, :1], pos[:, 1 + rng.permutation(63)[:7]]], axis=1).reshape(-1)
    what = f"copies/{dtype}/nq={nq}/split={split}"
    ids, _, st = search_case(va, oracle, raw, rq, 10, dtype, "cosine", deleted, PATH_MFMA, split, what)
    for g in range(nq):
        survivors = np.sort(np.setdiff1d(pos[g], deleted))
        assert np.array_equal(ids[g], survivors[:10].astype(np.uint64)), what
    assert st["band_queries"] > 0, f"{what}: {st}"


# ---------------------------------------------------------------- edges
N_SMALL, D_SMALL = 40_000, 48
EDGE_PATHS = [("bf16", 3, PATH_STREAM), ("f32", 3, PATH_STREAM), ("bf16", 300, PATH_MFMA), ("f32", 40, PATH_MFMA),
              ("f32", 5, PATH_EXACT)]


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(99)
    return rng.standard_normal((N_SMALL, D_SMALL)).astype(np.float32), rng.standard_normal((300, D_SMALL)).astype(np.float32)


@pytest.mark.parametrize("dtype,nq,path", EDGE_PATHS)
@pytest.mark.parametrize("kind", ["ninety", "k_minus_3", "all"])
def test_heavy_deletions(va, oracle, small, dtype, nq, path, kind):
    raw, queries = small
    rng = np.random.default_rng(3)
    k = 10
    if kind == "ninety":
        deleted = rng.choice(N_SMALL, N_SMALL * 9 // 10, replace=False)
    elif kind == "k_minus_3":
        deleted = np.setdiff1d(np.arange(N_SMALL), rng.choice(N_SMALL, k - 3, replace=False))
    else:
        deleted = np.arange(N_SMALL)
    what = f"{kind}/{dtype}/nq={nq}/path={path}"
    ids, sc, _ = search_case(va, oracle, raw, queries[:nq], k, dtype, "cosine", deleted, path, None, what)
    if kind == "k_minus_3":
        assert (ids[:, k - 3:] == ID_NONE).all() and np.isnan(sc[:, k - 3:]).all(), what
        assert (ids[:, :k - 3] != ID_NONE).all(), what
    if kind == "all":
        assert (ids == ID_NONE).all() and np.isnan(sc).all(), what


def test_repeats_errors_add_and_live_count(va, oracle, small):
    raw, queries = small
    rq = queries[:4]
    k = 8
    with va.Index(D_SMALL, "f32", "l2") as ix:
        ix.add(raw)
        assert ix.live_count() == N_SMALL
        ix.delete([])                                # n == 0: nothing
        ix.delete(np.array([5, 5, 9], dtype=np.int32))   # twice in one call
        ix.delete([5])                               # again
        assert ix.live_count() == N_SMALL - 2
        ids, sc = ix.search(rq, k)
        oi, osc = oracle_live(oracle, raw, rq, k, "f32", "l2", [5, 9])
        assert_same(ids, sc, oi, osc, "repeats")
        # an id that is not a row fails the whole call: nothing is deleted, the next search gives the same bits
        for bad in ([7, N_SMALL], [N_SMALL + 100], [1, 2, 2**63]):
            with pytest.raises(va.VrodError) as e:
                ix.delete(bad)
            assert e.value.code == 1
        assert ix.live_count() == N_SMALL - 2
        ids2, sc2 = ix.search(rq, k)
        assert np.array_equal(ids2, ids) and np.array_equal(bits(sc2), bits(sc))
        # add after delete: ids continue from count, the new rows are searchable and deletable
        more = np.ascontiguousarray(rq * 1.5)        # the queries' own best matches (L2)
        ix.add(more)
        assert ix.count == N_SMALL + 4 and ix.live_count() == N_SMALL + 2
        full = np.concatenate([raw, more])
        ids, sc = ix.search(rq, k)
        oi, osc = oracle_live(oracle, full, rq, k, "f32", "l2", [5, 9])
        assert_same(ids, sc, oi, osc, "after add")
        ix.delete([N_SMALL + 1, N_SMALL + 3])
        ids, sc = ix.search(rq, k)
        oi, osc = oracle_live(oracle, full, rq, k, "f32", "l2", [5, 9, N_SMALL + 1, N_SMALL + 3])
        assert_same(ids, sc, oi, osc, "after add + delete")
        # get_rows still reads deleted rows back
        assert np.array_equal(ix.get_rows(5, 1)[0], raw[5])


@pytest.mark.parametrize("nq,path", [(3, PATH_STREAM), (300, PATH_MFMA), (3, PATH_EXACT)])
def test_id_offset(va, oracle, small, nq, path):
    raw, queries = small
    off = 1_000_000
    rq = queries[:nq]
    with va.Index(D_SMALL, "bf16", "ip") as ix:
        ix.set_id_offset(off)
        ix.add(raw)
        ix.set_path(path)
        for bad in ([0], [off - 1], [off + N_SMALL]):
            with pytest.raises(va.VrodError):
                ix.delete(bad)
        deleted = np.arange(0, N_SMALL, 7)
        ix.delete(deleted + off)
        ids, sc = ix.search(rq, 10)
        assert ix.live_count() == N_SMALL - deleted.size
    oi, osc = oracle_live(oracle, raw, rq, 10, "bf16", "ip", deleted, id_offset=off)
    assert_same(ids, sc, oi, osc, f"offset/nq={nq}/path={path}")


# ---------------------------------------------------------------- a deleted prefix: the sample window
def test_deleted_prefix_keeps_the_certificates(va):
    """The first 30 % of a 1M x 768 bf16 corpus deleted, batch 1024: the sample pass must find its threshold on live
    rows, else every row of the first stage is a hit and every query ends on the exact path.  Reference: a handle
    that holds only the live rows (id offset = their first id), searched on the exact path."""
    import torch
    n, dim, nq, k, cut = 1_000_000, 768, 1024, 10, 300_000
    dev = torch.device("cuda", 0)
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    osc = torch.empty((nq, k), dtype=torch.float32, device=dev)
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add_synthetic(11, 0, n)
        ix.delete(np.arange(cut))
        assert ix.live_count() == n - cut
        ix.search_synthetic_device(12, 0, nq, k, oi, osc)
        torch.cuda.synchronize()
        st = ix.last_stats()
        ids, sc = oi.cpu().numpy().view(np.uint64), osc.cpu().numpy()
    assert st["path"] == PATH_MFMA and st["fallback_queries"] == 0, st
    check_bound(st, "prefix")
    with va.Index(dim, "bf16", "cosine") as ref:
        ref.set_id_offset(cut)
        ref.add_synthetic(11, cut, n - cut)
        ref.set_path(PATH_EXACT)
        ref.search_synthetic_device(12, 0, nq, k, oi, osc)
        torch.cuda.synchronize()
        rid, rsc = oi.cpu().numpy().view(np.uint64), osc.cpu().numpy()
    assert_same(ids, sc, rid, rsc, "prefix")


# ---------------------------------------------------------------- pipelined form and graph replay
def test_delete_while_pending_fails_then_applies(va, oracle, small):
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
            ix.delete([0])
        assert e.value.code == 1
        ix.search_end()
        assert ix.live_count() == N_SMALL
        top = outs[0][0].cpu().numpy().view(np.uint64)[:, 0]
        deleted = np.unique(top).astype(np.int64)
        ix.delete(deleted)
        ix.search_begin_device(q, k, *outs[1])
        ix.search_end()
        torch.cuda.synchronize()
        ids, sc = outs[1][0].cpu().numpy().view(np.uint64), outs[1][1].cpu().numpy()
    oi, osc = oracle_live(oracle, raw, queries[:nq], k, "bf16", "cosine", deleted)
    assert_same(ids, sc, oi, osc, "pipelined")
    assert not np.isin(ids, deleted.astype(np.uint64)).any()


def test_graph_replay_sees_the_delete(va, oracle):
    """A small (<= 8 queries, <= 64 MB) search begun while another is pending with the same buffers is captured and
    replayed; a delete afterwards must reach the replayed search."""
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
        oi, osc = oracle_live(oracle, raw, rq, k, "f32", "cosine", [])
        for ids, sc in before:
            assert_same(ids, sc, oi, osc, "before")
        gone = [int(before[-1][0][0, 0]), int(before[-1][0][1, 3])]
        ix.delete(gone)
        after = pipeline(ix, 10)
        oi, osc = oracle_live(oracle, raw, rq, k, "f32", "cosine", gone)
        for step, (ids, sc) in enumerate(after):
            assert not np.isin(ids, np.array(gone, np.uint64)).any(), f"step {step}"
            assert_same(ids, sc, oi, osc, f"after, step {step}")
        ix.delete([int(after[-1][0][0, 0])])          # a second delete on a handle that already has a mask
        gone.append(int(after[-1][0][0, 0]))
        again = pipeline(ix, 8)
        oi, osc = oracle_live(oracle, raw, rq, k, "f32", "cosine", gone)
        for step, (ids, sc) in enumerate(again):
            assert_same(ids, sc, oi, osc, f"second delete, step {step}")


# ---------------------------------------------------------------- multi-device handle
@pytest.mark.parametrize("metric,nq,path", [("cosine", 3, PATH_STREAM), ("l2", 300, PATH_MFMA), ("ip", 3, PATH_EXACT)])
def test_multi_device_routes_deletions_to_shards(va, oracle, metric, nq, path):
    rng = np.random.default_rng(21)
    n, dim, k = 200_000, 32, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((nq, dim)).astype(np.float32)
    # both sides of the 65536-row block boundaries (shard 0 | shard 1 | shard 0 ...), and random rows
    deleted = np.unique(np.concatenate([np.arange(65530, 65542), np.arange(131068, 131076), rng.choice(n, 5000, replace=False)]))
    # plus the two best rows of every query, so that deletions decide its results
    with va.Index(dim, "f32", metric, devices=[0, 0]) as ix:
        ix.add(raw)
        ix.set_path(path)
        ids0, _ = ix.search(rq, k)
        deleted = np.unique(np.concatenate([deleted, ids0[:, :2].reshape(-1).astype(np.int64)]))
        ix.delete(deleted)
        assert ix.live_count() == n - deleted.size
        ids, sc = ix.search(rq, k)
    oi, osc = oracle_live(oracle, raw, rq, k, "f32", metric, deleted)
    assert_same(ids, sc, oi, osc, f"multi/{metric}/nq={nq}/path={path}")
