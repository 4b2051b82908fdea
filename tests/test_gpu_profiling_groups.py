"""Profiling changes nothing but the timings of a labelled, a tagged and a grouped search.

These three synchronous searches time their own score launches with event markers (and, through the wide groups, with the
ordinary search's events).  With profiling on they must return the same ids and score bits and report the same counters
as with it off; scan_ms is positive wherever a scan was launched, and zero with profiling off.

One corpus of 4 096 rows (d = 64) with five labels of 1, 37, 300, 1 000 and 2 758 rows; row r carries tag bit i when it
carries label i, so the five predicates {any: bit i} are as unequal.  24 queries spread over the five groups.  The
labelled and tagged searches run under PATH_GATHER (every group scored on its own rows: the segmented route) and under
PATH_MFMA (every group one masked ordinary search: the wide-group route); the grouped search runs under PATH_EXACT, where
every query takes its dense stage.  Each profiling level gets a fresh handle and the same calls in the same order, so
nothing a handle learns from one search (the candidate margin) separates the runs.
"""
import numpy as np
import pytest

from support import PATH_MFMA, PATH_EXACT, PATH_GATHER, va  # noqa: F401

pytestmark = pytest.mark.gpu

N, DIM, NQ, K = 4096, 64, 24, 10
SIZES = [1, 37, 300, 1000]                              # the fifth label owns the rest
TIMINGS = ("scan_ms", "total_ms", "sample_ms", "overlap_ms")


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(4096)
    raw = rng.standard_normal((N, DIM)).astype(np.float32)
    rq = rng.standard_normal((NQ, DIM)).astype(np.float32)
    group = np.full(N, len(SIZES), np.int64)
    perm, at = rng.permutation(N), 0
    for g, n in enumerate(SIZES):
        group[perm[at:at + n]] = g
        at += n
    labels = (group * 1_000_003 + 5).astype(np.uint32)
    tags = np.left_shift(np.uint64(1), group.astype(np.uint64))
    qgroup = np.array([0, 1, 2, 3, 4] * 3 + [4] * 6 + [1, 3, 3], np.int64)       # every group, 1 .. 9 queries each
    assert qgroup.size == NQ and np.unique(qgroup).size == 5
    qlabels = (qgroup * 1_000_003 + 5).astype(np.uint32)
    preds = np.zeros((NQ, 3), np.uint64)
    preds[:, 0] = np.left_shift(np.uint64(1), qgroup.astype(np.uint64))
    return raw, rq, labels, tags, qlabels, preds


def run(va, world, dtype, level, calls):
    """A fresh handle at profiling `level`: [(result arrays, stats)] of calls(ix), a list of (path, search) pairs."""
    raw, _, labels, tags, _, _ = world
    out = []
    with va.Index(DIM, dtype, "cosine") as ix:
        ix.add(raw)
        ix.set_labels(0, labels)
        ix.set_tags(0, tags)
        ix.set_profiling(level)
        for path, search in calls(ix):
            ix.set_path(path)
            res = search()
            out.append((res, ix.last_stats()))
    return out


def assert_only_timings_differ(off, on, what):
    assert len(off) == len(on)
    for i, ((r0, s0), (r1, s1)) in enumerate(zip(off, on)):
        print(what, i, s0, s1)
        for a, b in zip(r0, r1):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), f"{what} call {i}: results differ"
        for name in s0:
            if name not in TIMINGS:
                assert s0[name] == s1[name], f"{what} call {i}: {name} {s0[name]} != {s1[name]}"
        assert s0["scan_ms"] == 0, f"{what} call {i}: scan_ms with profiling off: {s0}"
        if s1["scan_launches"] > 0:
            assert s1["scan_ms"] > 0, f"{what} call {i}: no scan_ms with profiling on: {s1}"


@pytest.mark.parametrize("path", [PATH_GATHER, PATH_MFMA], ids=["gather", "mfma"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_labelled_and_tagged(va, world, dtype, path):
    _, rq, _, _, qlabels, preds = world

    def calls(ix):
        return [(path, lambda: ix.search_labeled(rq, K, qlabels)), (path, lambda: ix.search_tagged(rq, K, preds))]
    off = run(va, world, dtype, 0, calls)
    for (ids, _), st in off:
        assert (ids != np.uint64(0xFFFFFFFFFFFFFFFF)).sum() == NQ * K - 3 * (K - 1)    # the one-row group fills one slot
        assert st["scan_launches"] > 0 and st["nq"] == NQ and st["k"] == K
        assert (st["path"] == PATH_GATHER) == (path == PATH_GATHER)                  # the route this case is about
    for level in (1, 2):
        assert_only_timings_differ(off, run(va, world, dtype, level, calls), f"{dtype} path{path} level{level}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grouped_dense_stage(va, world, dtype):
    _, rq, _, _, _, _ = world

    def calls(ix):
        return [(PATH_EXACT, lambda: ix.search_grouped(rq, K))]
    off = run(va, world, dtype, 0, calls)
    (_, _, lab), st = off[0]
    assert st["path"] == PATH_EXACT and st["fallback_queries"] == NQ and st["scan_launches"] > 0
    assert all(np.unique(lab[q, :5]).size == 5 for q in range(NQ))                    # the five labels, once each
    for level in (1, 2):
        assert_only_timings_differ(off, run(va, world, dtype, level, calls), f"{dtype} grouped level{level}")
