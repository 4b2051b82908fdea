"""GPU tests of compaction (vrod_index_compact) against the CPU oracle and against a fresh handle.

The contract (DESIGN.md rule 12): after compact() the handle is indistinguishable, through the ABI, from a fresh handle
with the same id_offset to which only the surviving raw rows were added, in order: count == live_count, get_rows, every
search and range search (ids and score bits) -- and the scan_bytes / scan_flops / scan_launches of those searches,
which is the proof, without a clock, that deleted rows stopped costing scan time.
"""
import os

import numpy as np
import pytest

from support import (  # noqa: F401
    DT, METRIC_L2, PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, THREADS, va, bits, assert_same, check_bound, prep_of, form_of, eligible_rows, oracle_over)

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "l2", "ip"]
CHUNK = 65536          # compact_plan.h kCompactChunkRows: rows per staged chunk (rows of <= 4 KiB)


def test_chunk_constant_is_the_headers():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "vrod_amd", "csrc", "compact_plan.h")).read()
    assert int(re.search(r"kCompactChunkRows = 1u << (\d+);", src).group(1)) == 16 and CHUNK == 1 << 16


def oracle_rows(O, rows, rq, k, dtype, metric, id_offset=0, allowed=None):
    """The oracle over `rows` (ids 0.. + id_offset), or over its allowed rows with the ids mapped back."""
    return oracle_over(O, rows, rq, k, dtype, metric, eligible_rows(rows.shape[0], allowed), id_offset)


def numpy_map(n, deleted, offset=0):
    alive = np.ones(n, bool)
    alive[np.asarray(deleted, dtype=np.int64)] = False
    m = np.full(n, ID_NONE, np.uint64)
    m[alive] = np.arange(int(alive.sum()), dtype=np.uint64) + np.uint64(offset)
    return m, alive


STAT_KEYS = ("path", "scan_bytes", "scan_flops", "scan_launches", "split_pass", "nq", "k")


def same_cost(st, ref, what, fallbacks=True):
    for key in STAT_KEYS + (("fallback_queries",) if fallbacks else ()):
        assert st[key] == ref[key], f"{what}: {key}: {st[key]} != {ref[key]}"


# ---------------------------------------------------------------- every path x dtype x metric, 10 % deleted, staged corpus
N_BIG, D_BIG = 300_000, 64


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(2026)
    raw = rng.standard_normal((N_BIG, D_BIG)).astype(np.float32)
    deleted = np.sort(rng.choice(N_BIG, N_BIG // 10, replace=False))
    queries = rng.standard_normal((1024, D_BIG)).astype(np.float32)
    return raw, deleted, queries


CASES = [  # (dtype, nq, path, VROD_F32_SPLIT, the path the stats must report, split_pass): test_gpu_delete.py CASES
    ("f32", 3, PATH_STREAM, None, PATH_STREAM, 0),
    ("bf16", 3, PATH_STREAM, None, PATH_STREAM, 0),
    ("bf16", 40, PATH_MFMA, None, PATH_MFMA, 0),        # skinny
    ("bf16", 300, PATH_MFMA, None, PATH_MFMA, 0),       # 4-wave
    ("bf16", 1024, PATH_MFMA, None, PATH_MFMA, 0),
    ("f32", 300, PATH_MFMA, "0", PATH_MFMA, 0),         # fp32 phased
    ("f32", 300, PATH_MFMA, "1", PATH_MFMA, 1),         # bf16 split planes (built BEFORE the compaction)
    ("f32", 5, PATH_EXACT, None, PATH_EXACT, 0),
    ("bf16", 5, PATH_EXACT, None, PATH_EXACT, 0),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype,nq,path,split,want_path,want_split", CASES)
def test_compacted_handle_equals_a_fresh_one(va, oracle, big, metric, dtype, nq, path, split, want_path, want_split):
    from conftest import f32_split
    raw, deleted, queries = big
    rq = queries[:nq]
    what = f"{metric}/{dtype}/nq={nq}/path={path}/split={split}"
    want_map, alive = numpy_map(N_BIG, deleted)
    live = int(alive.sum())
    surv = np.ascontiguousarray(raw[alive])
    with f32_split(split), va.Index(D_BIG, dtype, metric) as ix:
        ix.add(raw)
        ix.set_path(path)
        ix.delete(deleted)
        ix.search(rq, 10)                            # with tombstones (and builds the planes of the split case)
        st_before = ix.last_stats()
        new_ids = ix.compact()
        assert ix.count == live and ix.live_count() == live and ix.filter_count() == live, what
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
        rows = ix.get_rows(0, live)
        with va.Index(D_BIG, dtype, metric) as ref:
            ref.add(surv)
            ref.set_path(path)
            ref.search(rq, 10)                       # the compacted handle has searched once before, too (k' history)
            rid, rsc = ref.search(rq, 10)
            rst = ref.last_stats()
    assert np.array_equal(new_ids, want_map), what
    oi, osc = oracle_rows(oracle, surv, rq, 10, dtype, metric)
    assert_same(ids, sc, oi, osc, what)
    assert_same(rid, rsc, oi, osc, what + "/fresh")
    check_bound(st, what)
    assert st["path"] == want_path and st["split_pass"] == want_split, what
    same_cost(st, rst, what)
    if path == PATH_EXACT:      # no fast scan: the exact path counts no scan work, before or after
        assert st["scan_bytes"] == st_before["scan_bytes"] == 0 and st["scan_flops"] == st_before["scan_flops"] == 0, f"{what}: {st_before} / {st}"
    else:
        assert st["scan_bytes"] < st_before["scan_bytes"] and st["scan_flops"] < st_before["scan_flops"], f"{what}: {st_before} / {st}"
    # the maximum row norm is taken afresh over the survivors: the bound is a fresh handle's
    assert np.array_equal(np.float32(st["eps_bound"]), np.float32(rst["eps_bound"]), equal_nan=True), f"{what}: {st} / {rst}"
    assert np.array_equal(bits(rows), bits(oracle.prepare(surv, DT[dtype], prep_of(metric), threads=THREADS))), f"{what}: get_rows"


# ---------------------------------------------------------------- deletion patterns: both chunk forms, the no-move prefix
N_PAT, D_PAT = 4 * CHUNK + 1234, 32      # several staged chunks


@pytest.fixture(scope="module")
def pat():
    rng = np.random.default_rng(55)
    return rng.standard_normal((N_PAT, D_PAT)).astype(np.float32), rng.standard_normal((300, D_PAT)).astype(np.float32)


def pattern(kind, n, rng):
    if kind == "prefix":            # all direct moves
        return np.arange(n * 3 // 10)
    if kind == "suffix":            # nothing moves
        return np.arange(n - n * 3 // 10, n)
    if kind == "alternate":         # staged, then direct
        return np.arange(0, n, 2)
    if kind == "row1":              # the gap never opens: every chunk staged
        return np.array([1])
    if kind == "all_but_7":
        return np.setdiff1d(np.arange(n), rng.choice(n, 7, replace=False))
    if kind == "all":
        return np.arange(n)
    if kind == "none":
        return np.zeros(0, np.int64)
    if kind == "random":
        return np.sort(rng.choice(n, n // 3, replace=False))
    raise ValueError(kind)


@pytest.mark.parametrize("dtype,nq,path", [("bf16", 300, PATH_MFMA), ("f32", 3, PATH_STREAM)])
@pytest.mark.parametrize("kind", ["prefix", "suffix", "alternate", "row1", "all_but_7", "all", "none", "random"])
def test_deletion_patterns(va, oracle, pat, kind, dtype, nq, path):
    raw, queries = pat
    rq = queries[:nq]
    k = 10
    what = f"{kind}/{dtype}/nq={nq}"
    deleted = pattern(kind, N_PAT, np.random.default_rng(9))
    want_map, alive = numpy_map(N_PAT, deleted, offset=500)
    live = int(alive.sum())
    surv = np.ascontiguousarray(raw[alive])
    with va.Index(D_PAT, dtype, "l2") as ix:
        ix.set_id_offset(500)
        ix.add(raw)
        ix.set_path(path)
        ix.delete(deleted + 500)
        new_ids = ix.compact()
        assert np.array_equal(new_ids, want_map), what
        assert ix.count == live and ix.live_count() == live, what
        ids, sc = ix.search(rq, k)
        if live:
            assert np.array_equal(bits(ix.get_rows(0, live)), bits(oracle.prepare(surv, DT[dtype], METRIC_L2, threads=THREADS))), what
        # add after compact: ids continue from the new count, the freed rows serve the add
        more = np.ascontiguousarray(queries[:5] * 1.001)
        ix.add(more)
        assert ix.count == live + 5 and ix.live_count() == live + 5, what
        ids2, sc2 = ix.search(rq, k)
    oi, osc = oracle_rows(oracle, surv, rq, k, dtype, "l2", id_offset=500)
    assert_same(ids, sc, oi, osc, what)
    if kind == "all_but_7":
        assert (ids[:, 7:] == ID_NONE).all() and np.isnan(sc[:, 7:]).all() and (ids[:, :7] != ID_NONE).all(), what
    if kind == "all":
        assert (ids == ID_NONE).all() and np.isnan(sc).all(), what
    oi, osc = oracle_rows(oracle, np.concatenate([surv, more]), rq, k, dtype, "l2", id_offset=500)
    assert_same(ids2, sc2, oi, osc, what + "/add after compact")
    m = min(nq, 5)
    assert (ids2[:m, 0] == np.arange(live, live + m, dtype=np.uint64) + np.uint64(500)).all(), what


# ---------------------------------------------------------------- sequences
N_SMALL, D_SMALL = 100_000, 48


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(97)
    return rng.standard_normal((N_SMALL, D_SMALL)).astype(np.float32), rng.standard_normal((300, D_SMALL)).astype(np.float32)


@pytest.mark.parametrize("dtype,nq,path", [("bf16", 300, PATH_MFMA), ("f32", 3, PATH_STREAM), ("f32", 5, PATH_EXACT)])
def test_delete_compact_twice_then_update(va, oracle, small, dtype, nq, path):
    raw, queries = small
    rq = queries[:nq]
    rng = np.random.default_rng(17)
    cur = raw
    with va.Index(D_SMALL, dtype, "cosine") as ix:
        ix.add(raw)
        ix.set_path(path)
        for rnd in range(2):
            ids0, _ = ix.search(rq, 10)
            deleted = np.unique(np.concatenate([rng.choice(cur.shape[0], cur.shape[0] // 4, replace=False), ids0[:, 0].astype(np.int64)]))
            ix.delete(deleted)
            m, alive = numpy_map(cur.shape[0], deleted)
            assert np.array_equal(ix.compact(), m)
            cur = np.ascontiguousarray(cur[alive])
            assert ix.count == cur.shape[0] == ix.live_count()
            ids, sc = ix.search(rq, 10)
            oi, osc = oracle_rows(oracle, cur, rq, 10, dtype, "cosine")
            assert_same(ids, sc, oi, osc, f"round {rnd}")
            assert np.array_equal(ix.compact(), np.arange(cur.shape[0], dtype=np.uint64))      # nothing deleted: the identity
        # update after compact: the ids are the new ones
        upd = np.sort(rng.choice(cur.shape[0], 3000, replace=False))
        rows = rng.standard_normal((upd.size, D_SMALL)).astype(np.float32)
        rows[:min(nq, 20)] = rq[:min(nq, 20)]
        with pytest.raises(va.VrodError) as e:
            ix.update([cur.shape[0]], rows[:1])                    # an old id past the new count
        assert e.value.code == 1
        ix.update(upd, rows)
        cur = cur.copy()
        cur[upd] = rows
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
        oi, osc = oracle_rows(oracle, cur, rq, 10, dtype, "cosine")
        assert_same(ids, sc, oi, osc, "update after compact")
        check_bound(st, "update after compact")


@pytest.mark.parametrize("dtype,nq,path,frac", [("bf16", 300, PATH_AUTO, 0.5), ("f32", 3, PATH_STREAM, 0.5), ("f32", 40, PATH_GATHER, 0.02),
                                                ("bf16", 300, PATH_GATHER, 0.3)])
def test_a_filter_follows_its_rows(va, oracle, small, dtype, nq, path, frac):
    raw, queries = small
    rq = queries[:nq]
    rng = np.random.default_rng(23)
    n_rows = N_SMALL - 777                           # the filter covers fewer rows than the handle holds
    allow = rng.random(n_rows) < frac
    deleted = np.sort(rng.choice(N_SMALL, N_SMALL // 5, replace=False))
    _, alive = numpy_map(N_SMALL, deleted)
    full = np.zeros(N_SMALL, bool)
    full[:n_rows] = allow
    surv = np.ascontiguousarray(raw[alive])
    new_allow = full[alive]
    with va.Index(D_SMALL, dtype, "ip") as ix:
        ix.add(raw)
        ix.set_filter(allow)
        ix.delete(deleted)
        ix.set_path(path)
        fc = ix.filter_count()
        ix.compact()
        assert ix.filter_count() == fc == int(new_allow.sum())
        assert ix.count == ix.live_count() == surv.shape[0]
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
        with va.Index(D_SMALL, dtype, "ip") as ref:
            ref.add(surv)
            ref.set_filter(new_allow)
            ref.set_path(path)
            rid, rsc = ref.search(rq, 10)
            rst = ref.last_stats()
        # rows added later are still not allowed; clearing the filter shows every survivor
        ix.add(np.ascontiguousarray(rq[:3] * 4.0))
        ids2, sc2 = ix.search(rq, 10)
        ix.set_filter(None)
        ids3, _ = ix.search(rq[:3], 1)
    what = f"filter/{dtype}/nq={nq}/path={path}/{frac}"
    oi, osc = oracle_rows(oracle, surv, rq, 10, dtype, "ip", allowed=new_allow)
    assert_same(ids, sc, oi, osc, what)
    assert_same(rid, rsc, oi, osc, what + "/fresh")
    same_cost(st, rst, what)
    assert_same(ids2, sc2, oi, osc, what + "/after add")
    assert np.array_equal(ids3[:, 0], np.arange(surv.shape[0], surv.shape[0] + 3, dtype=np.uint64)), what
    if path == PATH_GATHER:
        assert st["path"] == PATH_GATHER, st


@pytest.mark.parametrize("dtype,metric,nq", [("bf16", "cosine", 300), ("f32", "l2", 40), ("f32", "ip", 3)])
def test_range_search_after_compact(va, oracle, small, dtype, metric, nq):
    raw, queries = small
    rq = queries[:nq]
    rng = np.random.default_rng(43)
    deleted = np.sort(rng.choice(N_SMALL, N_SMALL // 3, replace=False))
    _, alive = numpy_map(N_SMALL, deleted)
    surv = np.ascontiguousarray(raw[alive])
    pc = oracle.prepare(surv, DT[dtype], prep_of(metric), threads=THREADS)
    pq = oracle.prepare(rq, DT[dtype], prep_of(metric), threads=THREADS)
    _, s30 = oracle.scan_topk(pc, pq, 30, form_of(metric), threads=THREADS)
    thr = s30[:, -1].copy()
    olims, oids, osc = oracle.scan_range(pc, pq, thr, form_of(metric), id_offset=9, threads=THREADS)
    with va.Index(D_SMALL, dtype, metric) as ix:
        ix.set_id_offset(9)
        ix.add(raw)
        ix.delete(deleted + 9)
        ix.range_search(rq, thr)
        ix.compact()
        lims, ids, sc = ix.range_search(rq, thr)
    assert np.array_equal(lims, olims), f"range/{dtype}/{metric}"
    assert np.array_equal(ids, oids) and np.array_equal(bits(sc), bits(osc)), f"range/{dtype}/{metric}"
    assert int(lims[-1]) >= 30 * nq


# ---------------------------------------------------------------- refusals: nothing changes
def test_pending_wrong_map_length_and_multi_device(va, oracle, small):
    import ctypes as C
    import torch
    raw, queries = small
    dev = torch.device("cuda", 0)
    nq, k = 300, 10
    q = torch.from_numpy(np.ascontiguousarray(queries[:nq])).to(dev)
    out = (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
    deleted = np.arange(0, N_SMALL, 3)
    with va.Index(D_SMALL, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.delete(deleted)
        ix.search_begin_device(q, k, *out)
        with pytest.raises(va.VrodError) as e:
            ix.compact()
        assert e.value.code == 1
        ix.search_end()
        torch.cuda.synchronize()
        ids0, sc0 = out[0].cpu().numpy().view(np.uint64).copy(), out[1].cpu().numpy().copy()
        buf = np.full(N_SMALL + 1, 77, np.uint64)
        for wrong in (N_SMALL - 1, N_SMALL + 1, 0):
            assert ix._L.vrod_index_compact(ix._h, buf.ctypes.data_as(C.c_void_p), wrong) == 1
        assert (buf == 77).all() and ix.count == N_SMALL and ix.live_count() == N_SMALL - deleted.size
        ids, sc = ix.search(queries[:nq], k)
        assert np.array_equal(ids, ids0) and np.array_equal(bits(sc), bits(sc0))
        assert ix._L.vrod_index_compact(ix._h, None, 0) == 0           # no map wanted
        assert ix.count == N_SMALL - deleted.size
    with va.Index(D_SMALL, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        ix.delete(deleted)
        ids0, sc0 = ix.search(queries[:nq], k)
        with pytest.raises(va.VrodError) as e:
            ix.compact()
        assert e.value.code == 6
        assert ix.count == N_SMALL and ix.live_count() == N_SMALL - deleted.size
        ids, sc = ix.search(queries[:nq], k)
        assert np.array_equal(ids, ids0) and np.array_equal(bits(sc), bits(sc0))


def test_graph_replay_before_and_after_a_compaction(va, oracle):
    """The pipeline of test_gpu_delete.py::test_graph_replay_sees_the_delete: graphs captured before a compaction hold
    the old row count and the old mask -- every step afterwards must give the compacted handle's results."""
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
        gone = np.unique(np.concatenate([np.arange(0, n, 5), before[-1][0][:, :2].reshape(-1).astype(np.int64)]))
        ix.delete(gone)
        pipeline(ix, 10)                              # graphs that hold the mask
        _, alive = numpy_map(n, gone)
        ix.compact()
        surv = np.ascontiguousarray(raw[alive])
        oi, osc = oracle_rows(oracle, surv, rq, k, "f32", "cosine")
        for step, (ids, sc) in enumerate(pipeline(ix, 10)):
            assert_same(ids, sc, oi, osc, f"after the compaction, step {step}")


# ---------------------------------------------------------------- at scale
def test_compaction_at_scale_keeps_the_certificates(va, oracle):
    """1M x 768 bf16 synthetic, 30 % deleted in a mixed pattern (a prefix, a stride, a block in the middle), batch
    1024.  Reference: a fresh handle over the survivors on the exact path (as test_gpu_delete.py
    test_deleted_prefix_keeps_the_certificates); the survivors are stretches of the synthetic stream."""
    import torch
    n, dim, nq, k = 1_000_000, 768, 1024, 10
    dead = np.zeros(n, bool)
    dead[:100_000] = True                   # a prefix
    dead[500_000:600_000] = True            # a block
    dead[200_000:400_000:2] = True          # every other row of a stretch
    assert int(dead.sum()) == 300_000
    deleted = np.flatnonzero(dead)
    dev = torch.device("cuda", 0)
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    osc = torch.empty((nq, k), dtype=torch.float32, device=dev)
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add_synthetic(11, 0, n)
        ix.delete(deleted)
        ix.search_synthetic_device(12, 0, nq, k, oi, osc)
        torch.cuda.synchronize()
        st_before = ix.last_stats()
        new_ids = ix.compact()
        assert ix.count == n - deleted.size == ix.live_count()
        ix.search_synthetic_device(12, 0, nq, k, oi, osc)
        torch.cuda.synchronize()
        st = ix.last_stats()
        ids, sc = oi.cpu().numpy().view(np.uint64), osc.cpu().numpy()
    want_map, alive = numpy_map(n, deleted)
    assert np.array_equal(new_ids, want_map)
    assert st["path"] == PATH_MFMA and st["fallback_queries"] == 0, st
    assert st["scan_bytes"] < 0.75 * st_before["scan_bytes"], (st_before, st)   # 70 % of the rows are left to scan
    check_bound(st, "scale")
    with va.Index(dim, "bf16", "cosine") as ref:
        # the survivors in order: synthetic rows are a function of (seed, row), so stretches are added as they are and
        # the strided stretch row by row in blocks through the host
        ref.add_synthetic(11, 100_000, 100_000)
        odd = np.arange(200_001, 400_000, 2)
        blk = oracle.synth_rows(11, 200_000, 200_000, dim, threads=THREADS)
        ref.add(np.ascontiguousarray(blk[1::2]))
        assert odd.size == blk[1::2].shape[0]
        ref.add_synthetic(11, 400_000, 100_000)
        ref.add_synthetic(11, 600_000, 400_000)
        assert ref.count == n - deleted.size
        ref.set_path(PATH_EXACT)
        ref.search_synthetic_device(12, 0, nq, k, oi, osc)
        torch.cuda.synchronize()
        rid, rsc = oi.cpu().numpy().view(np.uint64), osc.cpu().numpy()
    assert_same(ids, sc, rid, rsc, "scale")
