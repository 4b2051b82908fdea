"""The bottom layer of the test helpers: one definition of everything the test files share.

numpy and the CPU oracle only; torch and the library are imported inside the `va` fixture, so this module loads on a
machine without a GPU.  A test file takes what it needs with `from support import ...`; the fixtures `va` and `O` are
imported the same way (pytest finds a fixture in the importing module's namespace, so each file still gets its own
module-scoped instance).  index_model.py, the other *_model.py files and sequence_plans.py build on this module.
"""
import math
import os

import numpy as np
import pytest

# ---------------------------------------------------------------- the codes of include/vrod.h and of the oracle
DT = {"f32": 0, "bf16": 1}
ME = {"cosine": 0, "l2": 1}                        # the oracle's two score forms, by the name of the metric
METRIC_COSINE, METRIC_L2 = 0, 1
PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER = 0, 1, 2, 3, 4
ID_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_K = 3584                                       # VROD_MAX_K
THREADS = max(1, min(16, len(os.sched_getaffinity(0))))


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def va():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import vrod_amd
    vrod_amd.load()  # raises if the HIP library is missing: no fallback
    return vrod_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ---------------------------------------------------------------- comparing results bit for bit
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_f32(a, b):
    """Same shape, NaN in the same slots, the same bits everywhere else (so 0.0 is not -0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def assert_scores_same(sc, osc, what):
    sc, osc = np.asarray(sc), np.asarray(osc)
    assert sc.shape == osc.shape, f"{what}: score shapes differ, {sc.shape} != {osc.shape}"
    na, nb = np.isnan(sc), np.isnan(osc)
    assert np.array_equal(na, nb), f"{what}: NaN positions differ at {np.argwhere(na != nb)[:5]}"
    assert np.array_equal(bits(sc)[~na], bits(osc)[~nb]), f"{what}: score bits differ"


def assert_same(ids, sc, oi, osc, what=""):
    ids, oi = np.asarray(ids), np.asarray(oi)
    assert ids.shape == oi.shape, f"{what}: id shapes differ, {ids.shape} != {oi.shape}"
    assert np.array_equal(ids, oi), f"{what}: ids differ at {np.argwhere(ids != oi)[:5]}"
    assert_scores_same(sc, osc, what)


def assert_same_all_bits(ids, sc, oi, osc, what=""):
    """assert_same without the NaN rule: every score bit is compared, a NaN's payload included.  For results that hold
    no (ID_NONE, NaN) filler, or whose NaNs must be the oracle's own."""
    assert_same(ids, sc, oi, osc, what)
    assert np.array_equal(bits(sc), bits(osc)), f"{what}: score bits differ"


def check_bound(st, what):
    """Wherever a fast pass ran, the observed |fast - canonical| lies inside the bound the search reports."""
    if st["path"] != PATH_EXACT and np.isfinite(st["eps_bound"]):
        assert st["max_fast_err"] <= st["eps_bound"], f"{what}: {st}"


# ---------------------------------------------------------------- rows that try the ingest
def special_rows(n, dim, seed, src):
    """Rows that try the conversion: normal values, rows scaled by 2^+-10, fp16 subnormals, +-65504, -0.0, a zero row."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    if n >= 16:
        x[1] *= 1024.0
        x[2] /= 1024.0
        x[3] = 0.0                                            # an all-zero row (stays zero under cosine)
        x[4, ::2] = -0.0
        x[5, : min(dim, 8)] = (np.arange(1, min(dim, 8) + 1) * 2.0 ** -24).astype(np.float32)   # fp16 subnormals
        x[5, -1] = -(2.0 ** -24)
        x[6, 0], x[6, -1] = 65504.0, -65504.0                # the largest fp16 values
        x[7] = 1023 * 2.0 ** -24                              # the largest fp16 subnormal, a whole row
    return x


# ---------------------------------------------------------------- the oracle over a set of rows
def prep_of(metric):
    """How the oracle prepares rows and queries of a handle with `metric` (ip: the vectors as given, as l2)."""
    return METRIC_COSINE if metric == "cosine" else METRIC_L2


def form_of(metric):
    """How the oracle scores a pair (ip: the dot form, as cosine)."""
    return METRIC_L2 if metric == "l2" else METRIC_COSINE


def eligible_rows(n, allow=None, deleted=()):
    """The rows < n, ascending, that are allowed (allow: a bool array, rows past it are not; None: every row) and not
    deleted."""
    a = np.ones(n, bool)
    if allow is not None:
        a[:] = False
        a[:len(allow)] = allow
    a[np.asarray(deleted, dtype=np.int64)] = False
    return np.flatnonzero(a)


def oracle_over(O, raw, rq, k, dtype, metric, eligible, id_offset=0):
    """The oracle over the rows `eligible` (ascending positions) of `raw`, ids mapped back (+ id_offset)."""
    nq = rq.shape[0]
    if eligible.size == 0:
        return np.full((nq, k), ID_NONE, np.uint64), np.full((nq, k), np.nan, np.float32)
    pc = O.prepare(np.ascontiguousarray(raw[eligible]), DT[dtype], prep_of(metric), threads=THREADS)
    pq = O.prepare(rq, DT[dtype], prep_of(metric), threads=THREADS)
    i, s = O.scan_topk(pc, pq, k, form_of(metric), threads=THREADS)
    out = np.full(i.shape, ID_NONE, np.uint64)
    m = i != ID_NONE
    out[m] = eligible[i[m].astype(np.int64)].astype(np.uint64) + np.uint64(id_offset)
    return out, s


def drop_self(ids, sc, self_ids, k):
    """Each (k + 1)-list without the entry that carries the query's own id, cut to k."""
    oi = np.empty((ids.shape[0], k), np.uint64)
    osc = np.empty((ids.shape[0], k), np.float32)
    for q in range(ids.shape[0]):
        keep = np.flatnonzero(ids[q] != self_ids[q])[:k]
        assert keep.size == k
        oi[q], osc[q] = ids[q][keep], sc[q][keep]
    return oi, osc


def hard_thresholds(all_sc, metric):
    """Range thresholds from [nq, m] best-first scores.  Per query, cycling: exactly the score of the r-th result
    (r = 1, 10, 1000: the inclusive boundary), the midpoint between two neighbouring scores, and better than the best (an
    empty result among non-empty ones)."""
    nq, m = all_sc.shape
    thr = np.empty(nq, np.float32)
    for q in range(nq):
        kind = q % 5
        if kind < 3:
            thr[q] = all_sc[q, min((0, 9, 999)[kind], m - 1)]
        elif kind == 3:
            thr[q] = np.float32((np.float64(all_sc[q, 20]) + np.float64(all_sc[q, 21])) / 2)
        else:
            thr[q] = np.nextafter(all_sc[q, 0], np.float32(-np.inf if metric == "l2" else np.inf))
    return thr


# ---------------------------------------------------------------- host decisions of the library, restated
def row_bytes(dtype, dim):
    """Bytes of one stored row: the width is padded to 64 bf16 / 32 fp32 values (128 bytes either way)."""
    return (-(-dim // 64) * 64 * 2) if dtype == "bf16" else (-(-dim // 32) * 32 * 4)


def first_k(k, eligible):
    """Rows per query of the first round of the grouped searches (group_plan.h group_first_k, multivec_plan.h)."""
    return min(MAX_K, eligible, max(4 * k, k + 32))


def takes_segments(path, dtype, n, m, nq, dim):
    """search_plan.h filter_route and filter_cost, restated: whether nq queries over m eligible rows of n are scored on
    the eligible rows alone (the gather path, a label's or tag's own segment) and not by a dense masked scan."""
    if path == PATH_GATHER:
        return True
    if path != PATH_AUTO:
        return False
    if m == 0:
        return True
    rb = dim * (2.0 if dtype == "bf16" else 4.0)
    steps = float(nq) * dim
    masked = math.log10(n / m) if 0 < m < n else 0.0
    dense_step = (1.0e-6 if dtype == "bf16" else 3.0e-6) + 3.0e-7 * masked
    return m * (rb * 3.0e-4 + steps * 1.56e-4) < n * (rb * 2.0e-4 + steps * dense_step)
