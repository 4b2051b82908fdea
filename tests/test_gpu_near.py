"""GPU tests of near-duplicate detection (vrod_index_find_near_duplicates, _find_near_duplicates_device,
_delete_near_duplicates) against near_model: the CPU oracle's range scan over the rows get_rows reads back, and a
union-find in Python.

The corpus is 2,500 unit rows -- nine whole 256-row tiles and a ragged tail of 196, ten fp32 batches and three bf16
batches, the last of each partial -- in a shuffled order: 40 clusters of 2 to 30 noisy copies, three chains of five rows
in which neighbours qualify for each other at CHAIN_THR and rows two apart do not, singletons for the rest.  Everything is
exact: the map and the five exact stats equal the model's bit for bit at thresholds taken from the score set itself
(support.hard_thresholds: boundary ties occur) and at CHAIN_THR.  Of the diagnostics only splits > 0 under the small pool
is asserted, and pool_entries.
"""
import ctypes as C

import numpy as np
import pytest

import near_model
from near_model import ID_NONE, exact
from support import (DT, PATH_AUTO, PATH_EXACT, PATH_GATHER, O, assert_same, form_of, hard_thresholds, oracle_over, takes_segments,  # noqa: F401
                     va)

pytestmark = pytest.mark.gpu

N = 2500
OFF = 5000
BATCH = {"bf16": 1024, "f32": 256}                   # byid_plan.h: rows per batch of range queries
POOL_BUDGET = 1 << 22                                # near_plan.h kNearPoolBudget
ERR_INVALID_ARG, ERR_INVALID_VALUE, ERR_UNSUPPORTED = 1, 2, 6
CASES = [(dt, me, d) for dt in ("bf16", "f32") for me in ("cosine", "l2", "ip") for d in (64, 33)]
THETA = 0.2                                          # the angle between a chain's neighbours: cos 0.980, two apart 0.921


def chain_thr(metric):
    """Neighbours of a chain qualify (cos 0.980, squared distance 0.040), rows two apart do not (0.921, 0.158); the copies of
    a cluster do (cos > 0.99); bf16 rounding moves none of these by more than 0.01."""
    return np.float32(0.1 if metric == "l2" else 0.95)


def planted(dim, seed=1):
    rng = np.random.default_rng(seed * 100 + dim)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    rows, clusters, chains = [], [], []
    for size in rng.integers(2, 31, 40):
        base = unit(rng.standard_normal(dim))
        clusters.append(list(range(len(rows), len(rows) + int(size))))
        rows += [base] + [unit(base + 0.05 * unit(rng.standard_normal(dim))) for _ in range(int(size) - 1)]
    for _ in range(3):
        u = unit(rng.standard_normal(dim))
        v = rng.standard_normal(dim)
        v = unit(v - (v @ u) * u)
        chains.append(list(range(len(rows), len(rows) + 5)))
        rows += [np.cos(k * THETA) * u + np.sin(k * THETA) * v for k in range(5)]
    rows += list(unit(rng.standard_normal((N - len(rows), dim))))
    perm = rng.permutation(N)                                                    # row perm[i] of the handle is rows[i]
    x = np.empty((N, dim), np.float32)
    x[perm] = np.asarray(rows, np.float32)
    p = {"clusters": [sorted(int(perm[i]) for i in c) for c in clusters], "chains": [[int(perm[i]) for i in c] for c in chains]}
    used = {r for c in p["clusters"] + p["chains"] for r in c}
    p["single"] = [r for r in range(N) if r not in used]
    return x, p


@pytest.fixture(scope="module")
def worlds():
    return {d: planted(d) for d in (64, 33)}


def filled(va, worlds, dtype, metric, dim, off=0):
    x, p = worlds[dim]
    ix = va.Index(dim, dtype, metric)
    ix.reserve(N + 300)                                                          # the capacity exceeds the count
    ix.set_id_offset(off)
    ix.add(x)
    return ix, p


def score_thresholds(O, ix, metric, p):
    """Five thresholds out of the handle's own score set: the best-first scores of five stored rows against all stored
    rows (200 of them kept), through support.hard_thresholds."""
    rows = ix.get_rows(0, N)
    q = [p["clusters"][0][1], p["chains"][0][2], p["single"][0], p["single"][1], p["clusters"][3][0]]
    s = O.numpy_scores_canonical(rows, rows[q], form_of(metric))
    s = np.sort(s, axis=1) if metric == "l2" else -np.sort(-s, axis=1)
    return hard_thresholds(np.ascontiguousarray(s[:, :200]), metric)


# ---------------------------------------------------------------- 1: the map and the exact stats
@pytest.mark.parametrize("dtype,metric,dim", CASES)
def test_map_and_stats_equal_the_model(va, O, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim)
    with ix:
        thresholds = list(score_thresholds(O, ix, metric, p)) + [chain_thr(metric)]
        for thr in thresholds:
            want, wst = near_model.of_handle(O, ix, metric, thr)
            got, st = ix.find_near_duplicates(thr, stats=True)
            print(dtype, metric, dim, float(thr), st)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (thr, np.flatnonzero(got != want)[:8])
            assert exact(st) == wst and st["near_duplicates"] == st["rows"] - st["classes"] and st["rows"] == N, (thr, st, wst)
            assert st["pool_entries"] == POOL_BUDGET and st["batches"] >= -(-N // BATCH[dtype]) and st["splits"] == 0
        again, st2 = ix.find_near_duplicates(thr, stats=True)                    # a function of the handle's state and the threshold alone
        assert np.array_equal(again, got) and exact(st2) == exact(st)
        assert wst["largest_class"] >= 5 and 0 < wst["classes"] < N              # (the last threshold is CHAIN_THR: the planted classes)
        assert ix.live_count() == N and ix.count == N                            # a find deletes nothing


# ---------------------------------------------------------------- 2: chains
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 64), ("f32", "l2", 33), ("bf16", "ip", 33), ("f32", "cosine", 64)])
def test_chains_come_out_as_single_classes(va, O, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim, off=OFF)
    with ix:
        thr = chain_thr(metric)
        rows = ix.get_rows(0, N)
        out = ix.find_near_duplicates(thr)
        ok = (lambda s: s <= thr) if metric == "l2" else (lambda s: s >= thr)
        for chain in p["chains"]:
            s = O.numpy_scores_canonical(rows[chain], rows[chain], form_of(metric))
            assert all(ok(s[k, k + 1]) for k in range(4)) and not any(ok(s[k, j]) for k in range(5) for j in range(k + 2, 5))   # the premise
            assert np.all(out[chain] == np.uint64(min(chain) + OFF))             # single linkage: one class, its smallest id
            assert int((out == np.uint64(min(chain) + OFF)).sum()) == 5
        for cluster in p["clusters"]:
            assert np.all(out[cluster] == np.uint64(cluster[0] + OFF)) and int((out == np.uint64(cluster[0] + OFF)).sum()) == len(cluster)
        single = np.array(p["single"])
        assert np.array_equal(out[single], single.astype(np.uint64) + np.uint64(OFF))   # no neighbour: its own id


# ---------------------------------------------------------------- 3: the small pool
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 33), ("f32", "l2", 64), ("f32", "ip", 33), ("bf16", "l2", 64)])
def test_small_pool_splits_batches_and_changes_nothing(va, O, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim)
    with ix:
        rows = ix.get_rows(0, N)
        s = O.numpy_scores_canonical(rows, rows[p["single"][:1]], form_of(metric))[0]
        thr = np.sort(s)[29] if metric == "l2" else -np.sort(-s)[29]             # the 30th best score of a lone row: some 30 hits a row
        want, wst = near_model.of_handle(O, ix, metric, thr)
        assert wst["hits"] * BATCH[dtype] // N > N                               # a full batch's hits exceed a pool of N entries
        wide, st = ix.find_near_duplicates(thr, stats=True)
        small, sst = ix.find_near_duplicates(thr, small_pool=True, stats=True)
        print(dtype, metric, dim, float(thr), st, sst)
        assert np.array_equal(wide, want) and np.array_equal(small, want) and exact(st) == exact(sst) == wst
        assert st["splits"] == 0 and sst["splits"] > 0 and sst["pool_entries"] == N and sst["batches"] > st["batches"]
        both, _ = ix.find_near_duplicates(chain_thr(metric), small_pool=True, stats=True)
        assert np.array_equal(both, ix.find_near_duplicates(chain_thr(metric)))


# ---------------------------------------------------------------- 4: the paths
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 64), ("f32", "l2", 33), ("f32", "ip", 64)])
def test_exact_and_gather_paths_give_the_same_map(va, O, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim)
    with ix:
        thr = chain_thr(metric)
        want, wst = near_model.of_handle(O, ix, metric, thr)
        for path in (PATH_AUTO, PATH_EXACT, PATH_GATHER):
            ix.set_path(path)
            got, st = ix.find_near_duplicates(thr, stats=True)
            assert np.array_equal(got, want) and exact(st) == wst, path
            if path != PATH_AUTO:
                assert ix.last_stats()["path"] == path                           # honoured as by a range search


# ---------------------------------------------------------------- 5: deleted rows and filters
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 64), ("f32", "l2", 33), ("bf16", "ip", 33), ("f32", "cosine", 64)])
def test_only_eligible_rows_are_classed(va, O, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim, off=OFF)
    rng = np.random.default_rng(11)
    thr = chain_thr(metric)
    big = max(p["clusters"], key=len)
    dead = sorted({big[0], p["clusters"][1][0], p["chains"][0][2]} | {int(r) for r in rng.choice(p["single"], 200, replace=False)})
    dead_ids = np.array(dead, np.uint64) + np.uint64(OFF)
    with ix:
        ix.delete(dead_ids)
        want, wst = near_model.of_handle(O, ix, metric, thr, deleted=dead_ids)
        got, st = ix.find_near_duplicates(thr, stats=True)
        assert np.array_equal(got, want) and exact(st) == wst and st["rows"] == N - len(dead) == ix.live_count()
        assert np.all(got[dead] == ID_NONE) and got[big[1]] == big[1] + OFF      # the next live row is the class's smallest
        c = p["chains"][0]                                                       # without its middle row the chain is two pairs
        assert got[c[0]] == got[c[1]] == min(c[:2]) + OFF and got[c[3]] == got[c[4]] == min(c[3:]) + OFF
        # a wide filter: the dense masked scan
        wide = rng.random(N) < 0.85
        wide[p["chains"][1]] = [True, True, True, True, False]                   # a chain's end is not allowed: four rows are left
        ix.set_filter(wide)
        want, wst = near_model.of_handle(O, ix, metric, thr, allow=wide, deleted=dead_ids)
        got, st = ix.find_near_duplicates(thr, stats=True)
        m = ix.filter_count()
        assert not takes_segments(PATH_AUTO, dtype, N, m, min(BATCH[dtype], m), dim) and ix.last_stats()["path"] != PATH_GATHER
        assert np.array_equal(got, want) and exact(st) == wst and st["rows"] == m == wst["rows"]
        assert np.all(got[~wide] == ID_NONE) and int((got == got[p["chains"][1][0]]).sum()) == 4
        # a narrow filter: the gather route
        narrow = np.zeros(N, bool)
        narrow[big + p["chains"][2] + p["single"][:40]] = True
        ix.set_filter(narrow)
        want, wst = near_model.of_handle(O, ix, metric, thr, allow=narrow, deleted=dead_ids)
        got, st = ix.find_near_duplicates(thr, stats=True)
        m = ix.filter_count()
        assert m < 80 and takes_segments(PATH_AUTO, dtype, N, m, m, dim) and ix.last_stats()["path"] == PATH_GATHER
        assert np.array_equal(got, want) and exact(st) == wst and st["rows"] == m and st["batches"] == 1
        assert np.all(got[~narrow] == ID_NONE) and st["largest_class"] == len(big) - 1
        small, sst = ix.find_near_duplicates(thr, small_pool=True, stats=True)
        assert np.array_equal(small, want) and exact(sst) == wst and sst["pool_entries"] == m
        # the filter cleared: the deleted rows alone are left out again
        ix.set_filter(None)
        assert np.array_equal(ix.find_near_duplicates(thr), near_model.of_handle(O, ix, metric, thr, deleted=dead_ids)[0])


# ---------------------------------------------------------------- 6: the device form
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 33), ("f32", "l2", 64)])
def test_device_form_writes_the_same_map(va, worlds, dtype, metric, dim):
    import torch
    ix, p = filled(va, worlds, dtype, metric, dim, off=OFF)
    with ix:
        thr = chain_thr(metric)
        ix.delete(np.array(p["single"][:10], np.uint64) + np.uint64(OFF))
        want, wst = ix.find_near_duplicates(thr, stats=True)
        buf = torch.full((N + 1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        out, st = ix.find_near_duplicates_device(thr, out_first=buf)
        assert out is buf and np.array_equal(buf[:N].cpu().numpy().view(np.uint64), want) and exact(st) == exact(wst)
        assert int(buf[N]) == 0x5A5A5A5A                                         # the guard past count is untouched
        fresh, _ = ix.find_near_duplicates_device(thr, small_pool=True)
        assert np.array_equal(fresh[:N].cpu().numpy().view(np.uint64), want)
        assert int((want == ID_NONE).sum()) == 10


# ---------------------------------------------------------------- 7: refusals, the stats-only form, empty handles
def test_refusals_leave_the_outputs_alone(va, worlds):
    import torch
    from vrod_amd._lib import NearStats
    L = va.load()
    ix, p = filled(va, worlds, "bf16", "cosine", 33)
    thr = float(chain_thr("cosine"))
    nan = float("nan")

    def refused(h, code, threshold=thr, flags=0, device=False):
        """Both forms of find and the delete answer `code`; the map, the stats and the count are as they were."""
        out = np.full(N + 8, 7, np.uint64)
        st = NearStats(*([9] * 8))
        n = C.c_uint64(7)
        if device:
            d = torch.full((N + 8,), 7, dtype=torch.int64, device="cuda")
            assert L.vrod_index_find_near_duplicates_device(h._h, threshold, flags, d.data_ptr(), N, C.byref(st), None) == code
            assert bool((d == 7).all())
        else:
            assert L.vrod_index_find_near_duplicates(h._h, threshold, flags, out.ctypes.data_as(C.c_void_p), N, C.byref(st)) == code
        assert L.vrod_index_delete_near_duplicates(h._h, threshold, flags, C.byref(n)) == code
        assert np.all(out == 7) and all(getattr(st, f) == 9 for f, _ in NearStats._fields_)
        return n.value

    with ix:
        full, fst = ix.find_near_duplicates(thr, stats=True)
        st = NearStats(*([9] * 8))
        assert L.vrod_index_find_near_duplicates(ix._h, thr, 0, None, 0, C.byref(st)) == 0   # the stats-only form
        assert exact(st.as_dict()) == exact(fst) and st.rows == N
        assert L.vrod_index_find_near_duplicates(ix._h, thr, 0, None, 0, None) == 0
        for device in (False, True):
            for bad_len in (0, N - 1, N + 1, N + 8):
                st = NearStats(*([9] * 8))
                out = np.full(N + 8, 7, np.uint64)
                d = torch.full((N + 8,), 7, dtype=torch.int64, device="cuda")
                if device:
                    rc = L.vrod_index_find_near_duplicates_device(ix._h, thr, 0, d.data_ptr(), bad_len, C.byref(st), None)
                else:
                    rc = L.vrod_index_find_near_duplicates(ix._h, thr, 0, out.ctypes.data_as(C.c_void_p), bad_len, C.byref(st))
                assert rc == ERR_INVALID_ARG and np.all(out == 7) and bool((d == 7).all()) and st.rows == 9
            st = NearStats(*([9] * 8))
            assert L.vrod_index_find_near_duplicates(ix._h, thr, 0, None, N, C.byref(st)) == ERR_INVALID_ARG and st.rows == 9   # a length without a map
            assert refused(ix, ERR_INVALID_VALUE, threshold=nan, device=device) == 7             # a NaN threshold
            for flags in (1, 2, 0x40000000, 0x80000002, 0xFFFFFFFF):             # unknown flag bits
                assert refused(ix, ERR_INVALID_ARG, flags=flags, device=device) == 7
        assert ix.live_count() == N
        oi = torch.empty((4, 10), dtype=torch.int64, device="cuda")
        osc = torch.empty((4, 10), dtype=torch.float32, device="cuda")
        ix.search_begin_synthetic_device(2, 0, 4, 10, oi, osc)                   # a pending search
        for device in (False, True):
            assert refused(ix, ERR_INVALID_ARG, device=device) == 7
        ix.search_end()
        again, ast = ix.find_near_duplicates(thr, stats=True)
        assert ix.live_count() == N and np.array_equal(again, full) and exact(ast) == exact(fst)
        for inf in (np.inf, -np.inf):                                            # +-inf is allowed: nothing passes, or everything
            out, st = ix.find_near_duplicates(inf, stats=True)
            if inf > 0:
                assert np.array_equal(out, np.arange(N, dtype=np.uint64)) and st["hits"] == 0 and st["classes"] == N
            else:
                assert np.all(out == 0) and st["hits"] == N * (N - 1) and st["classes"] == 1 and st["largest_class"] == N
    devices = [0, 1] if torch.cuda.device_count() >= 2 else [0, 0]
    with va.Index(33, "bf16", "cosine", devices=devices) as two:                 # a multi-device handle
        two.add(worlds[33][0])
        for device in (False, True):
            assert refused(two, ERR_UNSUPPORTED, device=device) == 7
        assert two.live_count() == N


def test_empty_handles_give_zero_stats(va, worlds):
    zero = dict.fromkeys(("rows", "classes", "near_duplicates", "largest_class", "hits", "batches", "splits", "pool_entries"), 0)
    with va.Index(8, "f32", "l2") as empty:
        for _ in range(2):
            out, st = empty.find_near_duplicates(0.5, stats=True)
            assert out.size == 0 and st == zero and empty.delete_near_duplicates(0.5) == 0
            out, st = empty.find_near_duplicates_device(0.5)
            assert st == zero
            empty.reserve(500)
    x = worlds[33][0][:300]
    with va.Index(33, "bf16", "cosine") as ix:                                   # no eligible row: all deleted, then none allowed
        ix.add(x)
        ix.set_filter(np.zeros(300, bool))
        out, st = ix.find_near_duplicates(0.5, stats=True)
        assert out.size == 300 and np.all(out == ID_NONE) and st == zero and ix.delete_near_duplicates(-1.0) == 0
        ix.set_filter(None)
        ix.delete(np.arange(300, dtype=np.uint64))
        out, st = ix.find_near_duplicates(0.5, small_pool=True, stats=True)
        assert np.all(out == ID_NONE) and st == zero
        d, st = ix.find_near_duplicates_device(0.5)
        assert np.all(d[:300].cpu().numpy().view(np.uint64) == ID_NONE) and st == zero
        assert ix.delete_near_duplicates(0.5) == 0 and ix.live_count() == 0


# ---------------------------------------------------------------- 8: threshold 0 under L2 is find_duplicates
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_l2_threshold_zero_is_the_map_of_find_duplicates(va, dtype):
    """Squared distance <= 0 means every element equal as a number; without signed zeros (and without NaN) that is equal
    bits, and bit-identical rows chain no further."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal((700, 33)).astype(np.float32)
    assert not np.any(x == 0)
    x[300:340] = x[7]
    x[650:] = x[np.arange(50) * 3 + 1]
    x[5] = x[699]
    with va.Index(33, dtype, "l2") as ix:
        ix.set_id_offset(OFF)
        ix.add(x)
        ix.delete(np.array([7, 100], np.uint64) + np.uint64(OFF))
        want, dst = ix.find_duplicates(stats=True)
        got, st = ix.find_near_duplicates(0.0, stats=True)
        assert np.array_equal(got, want)
        assert (st["rows"], st["classes"], st["near_duplicates"], st["largest_class"]) == (dst["live"], dst["classes"], dst["duplicates"], dst["largest_class"])
        assert st["largest_class"] == 41 and got[300] == got[652] == 300 + OFF and got[7] == ID_NONE   # rows 300..339 and 652, row 7 deleted


# ---------------------------------------------------------------- 9: delete_near_duplicates
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 64), ("f32", "l2", 33), ("f32", "ip", 64)])
def test_delete_near_duplicates_keeps_the_smallest_id_of_each_class(va, O, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim, off=OFF)
    x = worlds[dim][0]
    thr = chain_thr(metric)
    rng = np.random.default_rng(31)
    allow = rng.random(N) < 0.9
    dead_ids = np.array(p["single"][:25], np.uint64) + np.uint64(OFF)
    rq = rng.standard_normal((6, dim)).astype(np.float32)
    rq[0] = x[p["clusters"][0][0]]
    with ix:
        ix.delete(dead_ids)
        ix.set_filter(allow)
        want, wst = near_model.of_handle(O, ix, metric, thr, allow=allow, deleted=dead_ids)
        live, elig = ix.live_count(), ix.filter_count()
        assert wst["near_duplicates"] > 300
        assert ix.delete_near_duplicates(thr) == wst["near_duplicates"]
        assert ix.live_count() == live - wst["near_duplicates"] and ix.filter_count() == elig - wst["near_duplicates"] == wst["classes"]
        ids = np.arange(N, dtype=np.uint64) + np.uint64(OFF)
        survivors = ids[want == ids]                                             # the smallest id of every model class
        out, st = ix.find_near_duplicates(thr, stats=True)
        assert np.array_equal(ids[out != ID_NONE], survivors) and np.array_equal(out[out != ID_NONE], survivors)
        assert st["near_duplicates"] == 0 and st["largest_class"] == 1 and st["rows"] == st["classes"] == wst["classes"] and st["hits"] == 0
        assert ix.delete_near_duplicates(thr) == 0 and ix.live_count() == live - wst["near_duplicates"]   # a second call deletes nothing
        # rows that were not eligible were never deleted: the filter lifted, they are live as before
        ix.set_filter(None)
        gone = np.concatenate([dead_ids - np.uint64(OFF), np.flatnonzero((want != ID_NONE) & (want != ids))]).astype(np.int64)
        assert ix.live_count() == N - gone.size
        ix.set_filter(allow)
        # an ordinary search afterwards equals the oracle over the survivors
        got_ids, got_sc = ix.search(rq, 10)
        assert_same(got_ids, got_sc, *oracle_over(O, x, rq, 10, dtype, metric, (survivors - np.uint64(OFF)).astype(np.int64), OFF), "after delete_near_duplicates")
