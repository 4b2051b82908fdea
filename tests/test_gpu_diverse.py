"""GPU tests of the diversified search (vrod_search_diverse, vrod_search_diverse_device) against its model.

The contract (include/vrod.h): per query the certified top `pool`, then min(k, filled) greedy MMR steps whose every
operation is one fp32 rounding -- so ids are compared for equality and the bits of scores and mmr for equality (a NaN
matches any NaN) with tests/diverse_model.py, which builds the pool with the CPU oracle, g with
oracle.numpy_scores_canonical and the greedy loop in explicit np.float32 steps.  Both calling forms run everywhere.

Corpus: 3000 rows -- 2500 Gaussian, 300 exact copies of some of them and 200 near-copies (the original + 1e-3 noise),
shuffled; half of the queries are corpus rows + 1e-2 noise, so that copies sit in their pools and pen ties exactly.
The model's pool and g depend on (queries, pool) only: they are computed once per shape and every (k, lambda) selects
from them.
"""
import ctypes as C

import numpy as np
import pytest

from diverse_model import DiverseModel
import support
from support import PATH_AUTO, PATH_EXACT, ID_NONE, va, bits, same_f32  # noqa: F401

pytestmark = pytest.mark.gpu

N = 3000
SENT_ID, SENT_SC, SENT_MM = np.uint64(0x5A5A5A5A5A5A5A5A), np.float32(-12345.5), np.float32(-777.25)


def assert_same(got, want, what=""):
    (ids, sc, mm), (oi, osc, omm) = got, want
    support.assert_same(ids, sc, oi, osc, what)
    assert same_f32(mm, omm), f"{what}: mmr bits differ at {np.argwhere(bits(mm) != bits(omm))[:5]}"


def raw_corpus(n, d, metric, seed):
    """n rows: 5/6 Gaussian, 1/10 exact copies, 1/15 near-copies (+ 1e-3 noise), shuffled."""
    rng = np.random.default_rng(seed)
    n_dup, n_near = n // 10, n // 15
    base = rng.standard_normal((n - n_dup - n_near, d)).astype(np.float32)
    if metric == "ip":   # norms spread over e^2, as the by-id tests spread them
        base *= np.exp(rng.uniform(-1.0, 1.0, (base.shape[0], 1))).astype(np.float32)
    dup = base[rng.integers(0, base.shape[0], n_dup)]
    near = base[rng.integers(0, base.shape[0], n_near)] + np.float32(1e-3) * rng.standard_normal((n_near, d)).astype(np.float32)
    raw = np.concatenate([base, dup, near.astype(np.float32)])
    return np.ascontiguousarray(raw[rng.permutation(n)])


def raw_queries(raw, nq, seed):
    rng = np.random.default_rng(seed)
    d = raw.shape[1]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    at = rng.integers(0, raw.shape[0], nq)
    nearq = raw[at] + np.float32(1e-2) * rng.standard_normal((nq, d)).astype(np.float32)
    q[::2] = nearq[::2]
    return q


_MODELS = {}


def model(d, dtype, metric, n=N):
    """(raw rows, the model holding them) of one shape: built once, shared, never mutated."""
    key = (n, d, dtype, metric)
    if key not in _MODELS:
        raw = raw_corpus(n, d, metric, 4000 + d)
        raw.setflags(write=False)
        m = DiverseModel(d, dtype, metric)
        m.add(raw)
        _MODELS[key] = (raw, m)
    return _MODELS[key]


def run_device(ix, q, k, pool, lam, want_mmr=True):
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()
    oi, osc, omm = ix.search_diverse_device(dq, k, pool, lam, want_mmr=want_mmr)
    return (oi.cpu().numpy().view(np.uint64), osc.cpu().numpy(), omm.cpu().numpy() if omm is not None else None)


def check_both_forms(ix, q, k, pool, lam, want, what):
    assert_same(ix.search_diverse(q, k, pool, lam), want, f"{what} host")
    st = ix.last_stats()
    assert st["k"] == k and st["nq"] == q.shape[0], st
    assert_same(run_device(ix, q, k, pool, lam), want, f"{what} device")


# (d, nq, pool, [(k, lambda), ...]): every dim, nq, (k, pool) pair and lambda of the contract's list
SHAPES = [
    (1, 3, 1, [(1, 0.5)]),
    (1, 70, 64, [(1, 0.3), (10, 0.5), (64, 0.0)]),
    (3, 70, 63, [(10, 0.5), (10, 0.0)]),
    (64, 3, 1024, [(100, 0.3)]),
    (64, 1, 64, [(64, 0.5), (10, 1.0)]),
    (100, 70, 65, [(10, 0.3), (10, 1.0)]),
    (100, 3, 64, [(10, 0.5), (1, 0.0)]),
    (768, 3, 257, [(20, 0.5), (20, 0.0), (20, 0.3)]),
    (768, 1, 64, [(10, 0.3)]),
]


@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_matches_the_model(va, dtype, metric):
    handles = {}
    try:
        for d, nq, pool, picks in SHAPES:
            raw, m = model(d, dtype, metric)
            if d not in handles:
                handles[d] = va.Index(d, dtype, metric)
                handles[d].add(raw)
            ix = handles[d]
            q = raw_queries(raw, nq, 100 * d + nq)
            pools = m.pools(q, pool)
            for k, lam in picks:
                want = m.select(pools, k, lam)
                check_both_forms(ix, q, k, pool, lam, want, f"d {d} nq {nq} k {k} pool {pool} lambda {lam}")
            if (d, nq) == (100, 70):   # the exact path as the first stage: the same bits
                ix.set_path(PATH_EXACT)
                k, lam = picks[0]
                assert_same(ix.search_diverse(q, k, pool, lam), m.select(pools, k, lam), "exact path")
                assert ix.last_stats()["path"] == PATH_EXACT
                ix.set_path(PATH_AUTO)
            if (d, nq) == (768, 3):    # no mmr buffer: ids and scores are the same, nothing else is written
                k, lam = picks[0]
                want = m.select(pools, k, lam)
                oi, osc, omm = run_device(ix, q, k, pool, lam, want_mmr=False)
                assert omm is None and np.array_equal(oi, want[0]) and same_f32(osc, want[1])
                assert (want[0] != ID_NONE).all() and not np.array_equal(want[0], pools[0][:, :k]), "lambda < 1 reorders this corpus"
    finally:
        for ix in handles.values():
            ix.close()


# ------------------------------------------------------------------ bulk ties: only the position rule decides
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bulk_ties_go_to_the_smaller_position(va, dtype, metric):
    rng = np.random.default_rng(31)
    raw = rng.integers(-1, 2, (500, 3)).astype(np.float32)       # 27 distinct rows: r, g and v tie in bulk
    q = rng.integers(-1, 2, (9, 3)).astype(np.float32)
    m = DiverseModel(3, dtype, metric)
    m.add(raw)
    with va.Index(3, dtype, metric) as ix:
        ix.add(raw)
        for pool, picks in ((64, [(20, 0.5), (64, 0.0), (20, 0.3)]), (200, [(50, 0.5), (7, 1.0)])):
            pools = m.pools(q, pool)
            sc = pools[1]
            assert (np.diff(sc, axis=1) == 0).mean() > 0.5, "premise: most neighbours in the pool tie"
            for k, lam in picks:
                check_both_forms(ix, q, k, pool, lam, m.select(pools, k, lam), f"ties pool {pool} k {k} lambda {lam}")


# ------------------------------------------------------------------ handle state: offset, deletes, filter, compact, short pools
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2"), ("f32", "ip")])
def test_offset_deletes_filter_and_compact(va, dtype, metric):
    d, off = 64, 1_000_003
    raw, _ = model(d, dtype, metric)
    rng = np.random.default_rng(77)
    q = raw_queries(raw, 5, 78)
    m = DiverseModel(d, dtype, metric, id_offset=off)
    m.add(raw)
    with va.Index(d, dtype, metric) as ix:
        ix.add(raw)
        ix.set_id_offset(off)
        dead = (rng.choice(N, 400, replace=False) + off).astype(np.uint64)
        allow = np.arange(N) % 3 == 0
        ix.delete(dead); m.delete(dead)
        ix.set_filter(allow); m.set_filter(allow)
        for pool, k, lam in ((100, 10, 0.5), (64, 64, 0.3)):
            want = m.search_diverse(q, k, pool, lam)
            assert (want[0][want[0] != ID_NONE] >= off).all()
            check_both_forms(ix, q, k, pool, lam, want, f"state pool {pool} k {k}")
        new_ids = ix.compact()
        assert np.array_equal(new_ids, m.compact())
        for pool, k, lam in ((100, 10, 0.5), (65, 20, 0.0)):
            check_both_forms(ix, q, k, pool, lam, m.search_diverse(q, k, pool, lam), f"compacted pool {pool} k {k}")
        # a filter that allows nothing: all-unfilled rows, and the queries are not looked at
        none = np.zeros(m.count, bool)
        ix.set_filter(none); m.set_filter(none)
        bad = q.copy()
        bad[1, 3] = np.nan
        got = ix.search_diverse(bad, 4, 8, 0.5)
        assert (got[0] == ID_NONE).all() and np.isnan(got[1]).all() and np.isnan(got[2]).all()
        assert_same(run_device(ix, bad, 4, 8, 0.5), got)


@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "l2")])
def test_pool_larger_than_the_eligible_rows(va, dtype, metric):
    d = 64
    raw, _ = model(d, dtype, metric)
    q = raw_queries(raw, 3, 5)
    m = DiverseModel(d, dtype, metric, id_offset=17)
    with va.Index(d, dtype, metric) as ix:
        ix.set_id_offset(17)
        got = ix.search_diverse(q, 50, 64, 0.5)                     # an empty handle
        assert (got[0] == ID_NONE).all() and np.isnan(got[1]).all() and np.isnan(got[2]).all()
        assert_same(run_device(ix, q, 50, 64, 0.5), got)
        ix.add(raw[:40]); m.add(raw[:40])
        want = m.search_diverse(q, 50, 64, 0.5)
        assert (want[0][:, :40] != ID_NONE).all() and (want[0][:, 40:] == ID_NONE).all()
        check_both_forms(ix, q, 50, 64, 0.5, want, "40 rows, pool 64, k 50")
        ix.delete(np.arange(17, 17 + 40, 2, dtype=np.uint64)); m.delete(np.arange(17, 17 + 40, 2, dtype=np.uint64))
        want = m.search_diverse(q, 50, 64, 0.3)
        assert (want[0][:, 20:] == ID_NONE).all() and (want[0][:, :20] != ID_NONE).all()
        check_both_forms(ix, q, 50, 64, 0.3, want, "20 live rows, pool 64, k 50")


# ------------------------------------------------------------------ widths: the LDS budget's far end, and a dim that is no multiple of 64
@pytest.mark.parametrize("d,dtype,metric,n,nq,pool,k", [
    (32768, "bf16", "cosine", 300, 1, 256, 20),    # (one query: the model's g is a 32768-step numpy loop over 256 x 256)
    (32768, "f32", "l2", 300, 1, 256, 20),
    (4100, "bf16", "ip", 300, 3, 65, 10),
    (4100, "f32", "cosine", 300, 3, 65, 10),
])
def test_wide_rows(va, d, dtype, metric, n, nq, pool, k):
    raw, m = model(d, dtype, metric, n=n)
    q = raw_queries(raw, nq, 9)
    pools = m.pools(q, pool)
    with va.Index(d, dtype, metric) as ix:
        ix.add(raw)
        for lam in (0.5, 0.0):
            check_both_forms(ix, q, k, pool, lam, m.select(pools, k, lam), f"d {d} lambda {lam}")


# ------------------------------------------------------------------ lambda = 1 is the plain search
@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "cosine"), ("f32", "l2"), ("bf16", "ip")])
def test_lambda_one_is_the_plain_search(va, dtype, metric):
    d = 100
    raw, _ = model(d, dtype, metric)
    q = raw_queries(raw, 70, 3)
    with va.Index(d, dtype, metric) as ix:
        ix.add(raw)
        for k, pool in ((10, 64), (33, 33), (1, 1024)):
            oi, osc = ix.search(q, k)
            ids, sc, mm = ix.search_diverse(q, k, pool, 1.0)
            assert np.array_equal(ids, oi) and np.array_equal(bits(sc), bits(osc)), (k, pool)
            assert np.array_equal(mm, sc)
            di, ds, _ = run_device(ix, q, k, pool, 1.0)
            assert np.array_equal(di, oi) and np.array_equal(bits(ds), bits(osc)), (k, pool)


# ------------------------------------------------------------------ refusals: the outputs are not touched
def test_refusals_leave_the_outputs_untouched(va):
    import torch
    L = va.load()
    d = 64
    raw, _ = model(d, "f32", "cosine")
    q = raw_queries(raw, 4, 1)
    k, pool = 5, 16
    ids = np.full((4, k), SENT_ID, np.uint64)
    sc = np.full((4, k), SENT_SC, np.float32)
    mm = np.full((4, k), SENT_MM, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d_ids = torch.full((4, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    d_sc = torch.full((4, k), float(SENT_SC), dtype=torch.float32, device="cuda")
    d_mm = torch.full((4, k), float(SENT_MM), dtype=torch.float32, device="cuda")

    def host(h, qq=q, kk=k, pp=pool, lam=0.5):
        return L.vrod_search_diverse(h, p(qq), 4, kk, pp, lam, p(ids), p(sc), p(mm))

    def device(ix, qq=q, kk=k, pp=pool, lam=0.5):
        with pytest.raises(va.VrodError) as e:
            ix.search_diverse_device(torch.from_numpy(qq).cuda(), kk, pp, lam, out_ids=d_ids, out_scores=d_sc, out_mmr=d_mm)
        return e.value.code

    def untouched():
        return ((ids == SENT_ID).all() and (sc == SENT_SC).all() and (mm == SENT_MM).all()
                and bool((d_ids == 0x5A5A5A5A5A5A5A5A).all()) and bool((d_sc == float(SENT_SC)).all()) and bool((d_mm == float(SENT_MM)).all()))

    with va.Index(d, "f32", "cosine") as ix:
        ix.add(raw)
        # the arguments alone
        for kk, pp, lam in ((0, 16, 0.5), (17, 16, 0.5), (5, 1025, 0.5), (5, 16, float("nan")), (5, 16, -0.5), (5, 16, 1.5)):
            assert host(ix._h, kk=kk, pp=pp, lam=lam) == 1 and device(ix, kk=kk, pp=pp, lam=lam) == 1
        assert L.vrod_search_diverse(ix._h, None, 4, k, pool, 0.5, p(ids), p(sc), p(mm)) == 1
        assert L.vrod_search_diverse(ix._h, p(q), 4, k, pool, 0.5, None, p(sc), p(mm)) == 1
        assert L.vrod_search_diverse(ix._h, p(q), 4, k, pool, 0.5, p(ids), None, p(mm)) == 1
        assert L.vrod_search_diverse(ix._h, None, 0, k, pool, 0.5, None, None, None) == 0        # nq == 0
        # NaN / Inf in the queries: refused by the first stage, before the selection writes
        for v in (np.nan, np.inf):
            bad = q.copy()
            bad[2, 7] = v
            assert host(ix._h, qq=bad) == 2 and device(ix, qq=bad) == 2
        assert untouched()
        # while a search is pending
        dq = torch.from_numpy(q[:2].copy()).cuda()
        oi = torch.empty((2, 4), dtype=torch.int64, device="cuda")
        os_ = torch.empty((2, 4), dtype=torch.float32, device="cuda")
        ix.search_begin_device(dq, 4, oi, os_)
        try:
            assert host(ix._h) == 1 and device(ix) == 1
        finally:
            ix.search_end()
        assert untouched()
        # ... and the handle still answers
        got = ix.search_diverse(q, k, pool, 0.5)
        assert (got[0] != ID_NONE).all()
    # a multi-device handle (a repeated device id, as tests/test_gpu_multidevice.py makes them)
    with va.Index(d, "f32", "cosine", devices=[0, 0]) as mix:
        mix.add(raw[:300])
        assert host(mix._h) == 6 and device(mix) == 6
    assert untouched()
