"""GPU tests of the range search (vrod_range_search) against the CPU oracle.

The contract (DESIGN.md scan spec, rule 10): with `elig` the increasing list of eligible rows (live, and allowed while a
filter is set), ids, sc = scan_topk(prepared[elig], pq, len(elig), metric); query q's answer is the prefix of row q whose
scores satisfy  s >= threshold[q]  (cosine, ip)  /  s <= threshold[q]  (l2) -- a NaN score never does -- ids mapped
through elig.  lims, ids and score bits must be the oracle's, and wherever a fast pass ran the observed |fast - canonical|
must lie inside the bound the search reports.
"""
import functools

import numpy as np
import pytest

from conftest import f32_split
from support import DT, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, THREADS, va, bits, assert_same_all_bits, hard_thresholds  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_CAPACITY = 1, 8
METRICS = ["cosine", "l2", "ip"]
# (handle dtype, VROD_F32_SPLIT): fp32 over the bf16 planes, fp32 on the fp32 matrix pass, bf16
FORMS = [("f32", "1"), ("f32", "0"), ("bf16", None)]


def better(metric):
    return np.less_equal if metric == "l2" else np.greater_equal


def oracle_scores(O, raw, rq, dtype, metric, elig=None):
    """Every eligible row of every query, best first: (ids through elig [nq, m], scores [nq, m])."""
    prep = 0 if metric == "cosine" else 1
    scan = 1 if metric == "l2" else 0
    elig = np.arange(raw.shape[0]) if elig is None else np.asarray(elig)
    nq = rq.shape[0]
    if elig.size == 0:
        return np.zeros((nq, 0), np.uint64), np.zeros((nq, 0), np.float32)
    pc = O.prepare(np.ascontiguousarray(raw[elig]), DT[dtype], prep, threads=THREADS)
    pq = O.prepare(rq, DT[dtype], prep, threads=THREADS)
    ids, sc = O.scan_topk(pc, pq, elig.size, scan, threads=THREADS)
    return elig.astype(np.uint64)[ids.astype(np.int64)], sc


def oracle_range(all_ids, all_sc, thr, metric, id_offset=0):
    lims, oi, osc = [0], [], []
    with np.errstate(invalid="ignore"):
        for q in range(all_sc.shape[0]):
            ok = better(metric)(all_sc[q], np.float32(thr[q]))      # NaN scores: False
            n = int(ok.sum())
            assert ok[:n].all(), "qualifying rows are a prefix of the best-first order"
            oi.append(all_ids[q, :n] + np.uint64(id_offset))
            osc.append(all_sc[q, :n])
            lims.append(lims[-1] + n)
    return np.array(lims, np.uint64), np.concatenate(oi) if oi else np.zeros(0, np.uint64), np.concatenate(osc) if osc else np.zeros(0, np.float32)


def assert_range(got, want, what=""):
    (lims, ids, sc), (ol, oi, osc) = got, want
    assert np.array_equal(lims, ol), f"{what}: lims differ at {np.argwhere(lims != ol)[:5].ravel()} got {lims[:8]} want {ol[:8]}"
    assert_same_all_bits(ids, sc, oi, osc, what)


def check_stats(st, what, nq):
    print(what, {k: st[k] for k in ("path", "kprime", "scan_launches", "fallback_queries", "max_fast_err", "eps_bound")})
    assert st["k"] == 0 and st["nq"] == nq and st["band_queries"] == 0 and st["sample_ms"] == 0, f"{what}: {st}"
    if st["path"] == PATH_MFMA and st["fallback_queries"] < nq:
        assert np.isfinite(st["eps_bound"]) and st["max_fast_err"] <= st["eps_bound"], f"{what}: {st}"


# ---------------------------------------------------------------- the matrix: dtype x metric x batch size
N_ROWS, DIM = 5000, 96


@functools.lru_cache(maxsize=None)
def matrix_case(dtype, metric):
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(2024)
    raw = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    rq = rng.standard_normal((300, DIM)).astype(np.float32)
    return raw, rq, oracle_scores(O, raw, rq, dtype, metric)


@pytest.mark.parametrize("nq", [1, 5, 64, 65, 300])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype, split", FORMS)
def test_range_matches_oracle(va, oracle, dtype, split, metric, nq):
    raw, rq, (all_ids, all_sc) = matrix_case(dtype, metric)
    rq, all_ids, all_sc = rq[:nq], all_ids[:nq], all_sc[:nq]
    thr = hard_thresholds(all_sc, metric)
    with f32_split(split):
        with va.Index(DIM, dtype, metric) as ix:
            ix.add(raw)
            got = ix.range_search(rq, thr)
            st = ix.last_stats()
    assert_range(got, oracle_range(all_ids, all_sc, thr, metric), f"{dtype}/{split}/{metric}/{nq}")
    check_stats(st, f"{dtype}/{split}/{metric}/{nq}", nq)
    assert st["path"] == PATH_MFMA and st["scan_launches"] == 1 and st["fallback_queries"] == 0, st
    assert st["split_pass"] == (1 if split == "1" else 0), st


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_infinite_thresholds(va, oracle, dtype, metric):
    """Permissive side: every eligible row (NaN-scored IP rows excluded, none here); refusing side: nothing."""
    rng = np.random.default_rng(5)
    raw = rng.standard_normal((700, 40)).astype(np.float32)
    rq = rng.standard_normal((6, 40)).astype(np.float32)
    all_ids, all_sc = oracle_scores(oracle, raw, rq, dtype, metric)
    open_, shut = (np.inf, -np.inf) if metric == "l2" else (-np.inf, np.inf)
    thr = np.array([open_, shut, open_, all_sc[3, 4], shut, open_], np.float32)
    with va.Index(40, dtype, metric) as ix:
        ix.add(raw)
        got = ix.range_search(rq, thr)
        st = ix.last_stats()
    assert_range(got, oracle_range(all_ids, all_sc, thr, metric), f"{dtype}/{metric}")
    assert np.diff(got[0].astype(np.int64)).tolist() == [700, 0, 700, 5, 0, 700]
    check_stats(st, f"inf {dtype}/{metric}", 6)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_duplicated_row_at_the_threshold(va, oracle, dtype, metric):
    rng = np.random.default_rng(6)
    base = rng.standard_normal((3000, 64)).astype(np.float32)
    raw = np.concatenate([base[:1500], np.repeat(base[7:8], 300, axis=0), base[1500:]])
    rq = np.concatenate([base[7:8] + 0.5 * rng.standard_normal((1, 64)).astype(np.float32), rng.standard_normal((7, 64)).astype(np.float32)])
    all_ids, all_sc = oracle_scores(oracle, raw, rq, dtype, metric)
    dup_score = all_sc[0][all_ids[0] == 7][0]
    thr = np.full(8, dup_score, np.float32)
    with va.Index(64, dtype, metric) as ix:
        ix.add(raw)
        got = ix.range_search(rq, thr)
        st = ix.last_stats()
    want = oracle_range(all_ids, all_sc, thr, metric)
    assert_range(got, want, f"dup {dtype}/{metric}")
    tail = got[1][int(got[0][1]) - 301:int(got[0][1])].tolist()          # the 301 copies close query 0's segment, in id order
    assert tail == [7] + list(range(1500, 1800)), tail[:5]
    check_stats(st, f"dup {dtype}/{metric}", 8)


# ---------------------------------------------------------------- long results: split-and-redo, the long-segment sort
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype, split", FORMS)
def test_one_long_result_among_short_ones(va, oracle, dtype, split, metric):
    rng = np.random.default_rng(7)
    raw = rng.standard_normal((20000, 64)).astype(np.float32)
    rq = rng.standard_normal((12, 64)).astype(np.float32)
    all_ids, all_sc = oracle_scores(oracle, raw, rq, dtype, metric)
    tight = all_sc[:, 4].copy()
    loose = tight.copy()
    loose[3] = all_sc[3, 11999]        # 12000 rows: more than the 8192-entry lists and than VROD_MAX_K
    with f32_split(split):
        with va.Index(64, dtype, metric) as ix:
            ix.add(raw)
            got_l = ix.range_search(rq, loose)
            st_l = ix.last_stats()
            got_t = ix.range_search(rq, tight)
            st_t = ix.last_stats()
    assert_range(got_l, oracle_range(all_ids, all_sc, loose, metric), "loose")
    assert_range(got_t, oracle_range(all_ids, all_sc, tight, metric), "tight")
    assert int(got_l[0][4] - got_l[0][3]) == 12000
    check_stats(st_l, "loose", 12)
    check_stats(st_t, "tight", 12)
    assert st_l["scan_launches"] > 1 and st_t["scan_launches"] == 1, (st_l, st_t)


# ---------------------------------------------------------------- capacity, count-only, the handle afterwards
def test_capacity_and_count_only_and_search_afterwards(va, oracle):
    import ctypes as C
    rng = np.random.default_rng(8)
    raw = rng.standard_normal((5000, 96)).astype(np.float32)
    rq = rng.standard_normal((9, 96)).astype(np.float32)
    all_ids, all_sc = oracle_scores(oracle, raw, rq, "bf16", "cosine")
    thr = all_sc[:, 30].copy()
    want = oracle_range(all_ids, all_sc, thr, "cosine")
    total = int(want[0][-1])
    with va.Index(96, "bf16", "cosine") as ix:
        ix.add(raw)
        i0, s0 = ix.search(rq, 10)
        kp0 = ix.last_stats()["kprime"]
        assert_range(ix.range_search(rq, thr, capacity=total), want, "capacity == total")
        with pytest.raises(va.VrodError) as e:
            ix.range_search(rq, thr, capacity=total - 1)
        assert e.value.code == ERR_CAPACITY and np.array_equal(e.value.lims, want[0])
        # count-only: capacity 0, null outputs
        lims = np.zeros(10, np.uint64)
        rc = ix._L.vrod_range_search(ix._h, rq.ctypes.data_as(C.c_void_p), 9, thr.ctypes.data_as(C.c_void_p), 0,
                                     lims.ctypes.data_as(C.c_void_p), None, None)
        assert rc == ERR_CAPACITY and np.array_equal(lims, want[0])
        # entries past lims[-1] are not touched
        ids = np.full(total + 5, 12345, np.uint64)
        sc = np.full(total + 5, 7.0, np.float32)
        rc = ix._L.vrod_range_search(ix._h, rq.ctypes.data_as(C.c_void_p), 9, thr.ctypes.data_as(C.c_void_p), total + 5,
                                     lims.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p))
        assert rc == 0 and (ids[total:] == 12345).all() and (sc[total:] == 7.0).all()
        assert_range((lims, ids[:total], sc[:total]), want, "roomy")
        # nq = 0
        lims0 = np.full(1, 99, np.uint64)
        assert ix._L.vrod_range_search(ix._h, None, 0, None, 0, lims0.ctypes.data_as(C.c_void_p), None, None) == 0 and lims0[0] == 0
        # a NaN threshold
        bad = thr.copy()
        bad[2] = np.nan
        assert ix._L.vrod_range_search(ix._h, rq.ctypes.data_as(C.c_void_p), 9, bad.ctypes.data_as(C.c_void_p), 0,
                                       lims.ctypes.data_as(C.c_void_p), None, None) == 2
        # the handle answers a normal search afterwards: same bits, same k' (no margin or split-pass state was fed)
        i1, s1 = ix.search(rq, 10)
        assert np.array_equal(i0, i1) and np.array_equal(bits(s0), bits(s1)) and ix.last_stats()["kprime"] == kp0
        oi, osc = oracle.search(raw, rq, 10, 1, 0, threads=THREADS)
        assert np.array_equal(i1, oi) and np.array_equal(bits(s1), bits(osc))


@pytest.mark.parametrize("nq", [3, 200])
def test_topk_before_and_after_has_the_same_bits_and_kprime(va, oracle, nq):
    rng = np.random.default_rng(9)
    raw = rng.standard_normal((30000, 64)).astype(np.float32)
    rq = rng.standard_normal((nq, 64)).astype(np.float32)
    with va.Index(64, "bf16", "cosine") as ix:
        ix.add(raw)
        i0, s0 = ix.search(rq, 10)
        st0 = ix.last_stats()
        lims, _, _ = ix.range_search(rq, np.sort(s0, axis=1)[:, 0])      # each query's 10th best: ten rows each
        assert np.diff(lims.astype(np.int64)).min() >= 10
        i1, s1 = ix.search(rq, 10)
        st1 = ix.last_stats()
    assert np.array_equal(i0, i1) and np.array_equal(bits(s0), bits(s1))
    assert st0["kprime"] == st1["kprime"] and st0["path"] == st1["path"], (st0, st1)


def test_empty_handle(va):
    with va.Index(16, "f32", "l2") as ix:
        lims, ids, sc = ix.range_search(np.zeros((4, 16), np.float32), 1.0)
    assert lims.tolist() == [0] * 5 and ids.size == 0 and sc.size == 0


# ---------------------------------------------------------------- deleted rows and filters
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_delete_and_filter(va, oracle, dtype, metric):
    rng = np.random.default_rng(10)
    n, dim, nq = 6000, 64, 20
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((nq, dim)).astype(np.float32)
    deleted = rng.choice(n, 500, replace=False)
    dense = rng.random(n) < 0.6
    narrow = np.zeros(n, bool)
    narrow[rng.choice(n, 40, replace=False)] = True

    def elig(allow, dele):
        a = np.ones(n, bool) if allow is None else allow.copy()
        a[dele] = False
        return np.flatnonzero(a)

    def run(ix, e, want_path, what):
        all_ids, all_sc = oracle_scores(oracle, raw, rq, dtype, metric, e)
        m = all_sc.shape[1]
        thr = np.array([all_sc[q, min(m - 1, (0, 5, 37)[q % 3])] if m else 0.0 for q in range(nq)], np.float32)
        got = ix.range_search(rq, thr)
        st = ix.last_stats()
        assert_range(got, oracle_range(all_ids, all_sc, thr, metric, id_offset=100), what)
        check_stats(st, what, nq)
        assert st["path"] == want_path, (what, st)

    none = np.zeros(0, np.int64)
    with va.Index(dim, dtype, metric) as ix:
        ix.add(raw)
        ix.set_id_offset(100)
        ix.set_filter(dense)
        run(ix, elig(dense, none), PATH_MFMA, "dense filter")
        ix.set_filter(narrow)
        run(ix, elig(narrow, none), PATH_GATHER, "narrow filter")
        ix.set_filter(None)
        ix.delete(deleted + 100)
        run(ix, elig(None, deleted), PATH_MFMA, "deleted")
        ix.set_filter(dense)
        run(ix, elig(dense, deleted), PATH_MFMA, "deleted + dense filter")
        ix.set_filter(narrow)
        run(ix, elig(narrow, deleted), PATH_GATHER, "deleted + narrow filter")
        ix.set_filter(None)
        ix.delete(np.arange(n) + 100)
        lims, ids, sc = ix.range_search(rq, np.full(nq, -np.inf if metric != "l2" else np.inf, np.float32))
        assert lims.tolist() == [0] * (nq + 1) and ids.size == 0


# ---------------------------------------------------------------- the canonical route
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("path", [PATH_EXACT, PATH_STREAM])
def test_forced_paths(va, oracle, dtype, metric, path):
    """EXACT: canonical scores of every row, every query counted as a fallback.  STREAM has no threshold form: AUTO."""
    rng = np.random.default_rng(11)
    raw = rng.standard_normal((5000, 96)).astype(np.float32)
    rq = rng.standard_normal((11, 96)).astype(np.float32)
    all_ids, all_sc = oracle_scores(oracle, raw, rq, dtype, metric)
    thr = hard_thresholds(all_sc, metric)
    with va.Index(96, dtype, metric) as ix:
        ix.add(raw)
        ix.set_path(path)
        got = ix.range_search(rq, thr)
        st = ix.last_stats()
    assert_range(got, oracle_range(all_ids, all_sc, thr, metric), f"path {path}")
    check_stats(st, f"path {path}", 11)
    if path == PATH_EXACT:
        assert st["path"] == PATH_EXACT and st["fallback_queries"] == 11, st
    else:
        assert st["path"] == PATH_MFMA and st["fallback_queries"] == 0, st


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ip_bound_not_finite(va, oracle, dtype):
    """The inputs of the IP overflow tests: canonical scores include +inf, -inf and NaN, a squared row norm overflows,
    so no finite bound exists: every query takes the canonical route.  NaN-scored rows never qualify."""
    rng = np.random.default_rng(700)
    n, d = 2000, 8
    raw = rng.standard_normal((n, d)).astype(np.float32)
    pos = rng.choice(n, 150, replace=False)
    up, down, both = pos[:50], pos[50:100], pos[100:]
    raw[up, 0] = 1e20
    raw[down, 0] = -1e20
    raw[both, 0], raw[both, 1] = 1e20, -1e20
    q0 = np.ones(d, np.float32)
    q0[:2] = 1e20
    rq = np.stack([q0, np.zeros(d, np.float32), rng.standard_normal(d).astype(np.float32), -q0, q0 * np.float32(0.5),
                   rng.standard_normal(d).astype(np.float32) * 3]).astype(np.float32)
    all_ids, all_sc = oracle_scores(oracle, raw, rq, dtype, "ip")
    assert np.isnan(all_sc[0]).sum() == 50 and np.isposinf(all_sc[0]).any()
    thr = np.array([-np.inf, 0.0, all_sc[2, 10], np.inf, 1.0, -np.inf], np.float32)
    with va.Index(d, dtype, "ip") as ix:
        ix.add(raw)
        got = ix.range_search(rq, thr)
        st = ix.last_stats()
    want = oracle_range(all_ids, all_sc, thr, "ip")
    assert_range(got, want, "ip overflow")
    assert int(want[0][1]) == n - 50                      # -inf: every row but the NaN-scored ones
    assert st["fallback_queries"] == 6 and st["path"] == PATH_MFMA, st


@pytest.mark.parametrize("scale", [3e18, 1e19])
def test_l2_distances_that_overflow(va, oracle, scale):
    rng = np.random.default_rng(11)
    raw = (rng.standard_normal((9000, 96)) * scale).astype(np.float32)
    raw[17] = 0.0
    rq = (rng.standard_normal((5, 96)) * scale).astype(np.float32)
    rq[0] = 0.0
    all_ids, all_sc = oracle_scores(oracle, raw, rq, "f32", "l2")
    thr = np.array([0.0, np.inf, 3e38, all_sc[3, 0], np.inf], np.float32)
    with va.Index(96, "f32", "l2") as ix:
        ix.add(raw)
        got = ix.range_search(rq, thr)
        st = ix.last_stats()
    assert_range(got, oracle_range(all_ids, all_sc, thr, "l2"), f"l2 overflow {scale}")
    assert st["fallback_queries"] == 5, st


# ---------------------------------------------------------------- device entry point, pending searches
def test_device_entry_point_on_a_side_stream_and_pending_search(va, oracle):
    import torch
    rng = np.random.default_rng(12)
    raw = rng.standard_normal((8000, 64)).astype(np.float32)
    rq = rng.standard_normal((70, 64)).astype(np.float32)
    all_ids, all_sc = oracle_scores(oracle, raw, rq, "bf16", "l2")
    thr = all_sc[:, 14].copy()
    want = oracle_range(all_ids, all_sc, thr, "l2")
    total = int(want[0][-1])
    dev = torch.device("cuda:0")
    with va.Index(64, "bf16", "l2") as ix:
        ix.add(raw)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            dq = torch.from_numpy(rq).to(dev, non_blocking=True)
            dt = torch.from_numpy(thr).to(dev, non_blocking=True)
            rc, lims, ids, sc = ix.range_search_device(dq, dt, total)
            assert rc == 0
            rc2, lims2, _, _ = ix.range_search_device(dq, dt, total - 1)
            assert rc2 == ERR_CAPACITY
        side.synchronize()
        got = (lims.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint64)[:total], sc.cpu().numpy()[:total])
        assert_range(got, want, "device")
        assert np.array_equal(lims2.cpu().numpy().view(np.uint64), want[0])
        # a pending pipelined search: the range call fails and leaves that search intact
        oi = torch.empty((70, 10), dtype=torch.int64, device=dev)
        osc = torch.empty((70, 10), dtype=torch.float32, device=dev)
        dq0 = torch.from_numpy(rq).to(dev)
        dt0 = torch.from_numpy(thr).to(dev)
        torch.cuda.synchronize()
        ix.search_begin_device(dq0, 10, oi, osc)
        rc, _, _, _ = 0, None, None, None
        with pytest.raises(va.VrodError) as e:
            ix.range_search_device(dq0, dt0, total)
        assert e.value.code == ERR_INVALID_ARG
        with pytest.raises(va.VrodError) as e:
            ix.range_search(rq, thr)
        assert e.value.code == ERR_INVALID_ARG
        assert ix.pending == 1
        ix.search_end()
        ei, es = oracle.search(raw, rq, 10, 1, 1, threads=THREADS)
        assert np.array_equal(oi.cpu().numpy().view(np.uint64), ei) and np.array_equal(bits(osc.cpu().numpy()), bits(es))


# ---------------------------------------------------------------- multi-device handle
@pytest.mark.parametrize("metric", METRICS)
def test_two_shards_equal_one(va, oracle, metric):
    """devices=[0, 0]: rows are dealt in blocks of 65536, so 140000 rows put two blocks on shard 0 and one on shard 1.
    A row duplicated on both shards whose score is the threshold: tied scores across shards, merged by global id."""
    rng = np.random.default_rng(13)
    n, dim = 140000, 32
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    dup = raw[5].copy()
    for r in (100, 70000, 70001, 131080, 139999):       # shard 0, shard 1, shard 1, shard 0, shard 0
        raw[r] = dup
    rq = np.concatenate([dup[None] + 0.3 * rng.standard_normal((1, dim)).astype(np.float32), rng.standard_normal((6, dim)).astype(np.float32)])
    all_ids, all_sc = oracle_scores(oracle, raw, rq, "bf16", metric)
    thr = all_sc[:, 50].copy()
    thr[0] = all_sc[0][all_ids[0] == 5][0]
    thr[2] = all_sc[2, 9999]                              # a long segment across both shards
    want = oracle_range(all_ids, all_sc, thr, metric)
    with va.Index(dim, "bf16", metric) as ix:
        ix.add(raw)
        one = ix.range_search(rq, thr)
    with va.Index(dim, "bf16", metric, devices=[0, 0]) as ix:
        ix.add(raw)
        two = ix.range_search(rq, thr)
        st = ix.last_stats()
        with pytest.raises(va.VrodError) as e:
            ix.range_search(rq, thr, capacity=int(want[0][-1]) - 1)
        assert e.value.code == ERR_CAPACITY and np.array_equal(e.value.lims, want[0])
    assert_range(one, want, "one device")
    assert_range(two, want, "two shards")
    seg0 = two[1][:int(two[0][1])].tolist()
    assert seg0[-6:] == [5, 100, 70000, 70001, 131080, 139999], seg0[-8:]
    check_stats(st, "two shards", 7)
