"""GPU tests of group centroids (vrod_index_centroids_where) against centroid_model.CentroidModelIndex, bit for bit: the
group records, every bit of every vector and both counts.

The handles hold about 5000 rows -- two work-groups of 2048 rows and a tail (rowpred_plan.h), so one group is fed by
several work-groups and its sum goes through the atomics.  The widths are one lane (1), an odd tail (3), exactly one
16-byte piece of bf16 (8), no multiple of 8 (200), the bench width (768) and more pieces than a work-group has lanes on a
bf16 handle (1030 x 2 bytes: 129 pieces; fp32: 258).  The result is defined through an integer sum, so it may not depend
on the order of the rows: a second handle with the rows permuted must give the same bits, which float atomics would fail.
"""
import ctypes as C

import numpy as np
import pytest

from aggregate_model import BY_LABEL, BY_TAG, BY_VALUE
from centroid_model import CENTROID_GROUP_DTYPE, CENTROID_SUM, ERR_CAPACITY, MAX_CENTROID_GROUPS, CentroidModelIndex
from index_model import ModelError
from rowpred_model import ALLOWED, MATCH_ALL
from where_model import I64_MAX, I64_MIN
from support import va  # noqa: F401

pytestmark = pytest.mark.gpu

N = 5000
K = 10
SENT = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 6
F32_MAX = np.float32(3.4028234663852886e38)
FULL = (I64_MIN, I64_MAX)


# ---------------------------------------------------------------- label layouts
def documents(n, rng):
    """Contiguous runs of 1 to 40 rows, each run a label of its own."""
    runs = rng.integers(1, 41, n)
    return np.repeat(np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(5), runs)[:n]


LAYOUTS = {
    "one_label": lambda n, rng: np.full(n, 17, np.uint32),
    "documents": documents,
    "seven_random": lambda n, rng: rng.integers(0, 7, n).astype(np.uint32),
}


def make(va, rows, dtype, metric, off=0, labels=None, values=None, tags=None, reserve=300):
    """A handle of these raw rows reserved past its count, ids from `off`, and its model."""
    n, dim = rows.shape
    m = CentroidModelIndex(dim, dtype, metric, id_offset=off)
    ix = va.Index(dim, dtype, metric)
    ix.reserve(n + reserve)
    ix.set_id_offset(off)
    for h in (m, ix):
        h.add(rows)
        for setter, col in ((h.set_values, values), (h.set_labels, labels), (h.set_tags, tags)):
            if col is not None:
                setter(off, col)
    return ix, m


def raw_call(ix, pred, flags, by, width, capacity, room=None, stride=None, want=(True, True, True, True)):
    """The C entry point with sentinel-filled outputs -> (rc, count, rows, groups [room], vectors [room, stride])."""
    pp = pred if pred is None or isinstance(pred, np.ndarray) else ix._row_preds(pred, 1)
    room = max(int(capacity), 1) if room is None else room
    stride = ix.dim if stride is None else stride
    groups = np.full(room * 3, SENT, np.uint64).view(CENTROID_GROUP_DTYPE)
    vectors = np.full((room, stride if ix.dim <= stride <= ix.dim + 64 else ix.dim), SENT32, np.uint32)   # (a refused stride is never used)
    n, rows = C.c_uint64(SENT), C.c_uint64(SENT)
    rc = ix._L.vrod_index_centroids_where(ix._h, pp.ctypes.data if pp is not None else None, flags, by, width, capacity, C.byref(n) if want[0] else None,
                                          C.byref(rows) if want[1] else None, groups.ctypes.data if want[2] else None,
                                          vectors.ctypes.data if want[3] else None, stride)
    return rc, n.value, rows.value, groups, vectors


def untouched(*arrays):
    return all((a.view(np.uint32) == SENT32).all() for a in arrays)


def same(ix, m, pred, by, width=None, sums=False, allowed=False, pad=3, what=""):
    """One call equals the model: every field of every group, every bit of every vector, both counts; the floats between
    dim and the stride, and everything past the groups, keep their sentinel."""
    flags = (ALLOWED if allowed else 0) | (CENTROID_SUM if sums else 0)
    wg, wv, wr = m.centroids_where(pred, by, width, None, flags)
    tag = f"{what} dim{ix.dim} by{by} width{width} sums{sums} allowed{allowed}"
    cap = wg.size + 2
    rc, n, rows, groups, vectors = raw_call(ix, pred, flags, by, width or 0, cap, stride=ix.dim + pad)
    assert rc == 0 and (n, rows) == (wg.size, wr), f"{tag}: rc {rc}, groups {n} != {wg.size} or rows {rows} != {wr}"
    for name in CENTROID_GROUP_DTYPE.names:
        assert np.array_equal(groups[name][:n], wg[name]), f"{tag}: {name} differs at {np.flatnonzero(groups[name][:n] != wg[name])[:5]}"
    got = vectors[:n, :ix.dim]
    bad = np.argwhere(got != wv.view(np.uint32))
    assert bad.size == 0, f"{tag}: {bad.shape[0]} vector elements differ, first at {bad[:3].tolist()}: {got[tuple(bad[0])]:#x} != {wv.view(np.uint32)[tuple(bad[0])]:#x}"
    assert untouched(vectors[:, ix.dim:], vectors[n:], groups[n:]), f"{tag}: padding or the entries past the groups were written"
    assert rows == ix.count_where([pred], allowed)[0], tag
    return wg, wv


# ---------------------------------------------------------------- widths x storage x metric x layouts
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("dim", [1, 3, 8, 200, 768, 1030])
def test_widths_metrics_and_label_layouts(va, dim, dtype):
    rng = np.random.default_rng(dim * 7 + len(dtype))
    rows = rng.standard_normal((N, dim)).astype(np.float32)
    rows[::9] *= np.float32(37.5)
    rows[5] = 0.0                                                                # a zero row stays zero under cosine
    values = rng.integers(-60, 60, N).astype(np.int64)
    for i, metric in enumerate(("cosine", "l2", "ip")):
        layout = list(LAYOUTS)[(i + dim) % 3]
        ix, m = make(va, rows, dtype, metric, off=1000 * (i % 2), labels=LAYOUTS[layout](N, rng), values=values)
        with ix:
            for sums in (False, True):
                wg, _ = same(ix, m, MATCH_ALL, BY_LABEL, sums=sums, what=f"{metric} {layout}")
            assert int(wg["count"].sum()) == N
            other = list(LAYOUTS)[(i + dim + 1) % 3]
            relabel = LAYOUTS[other](N, rng)
            for h in (ix, m):
                h.set_labels(1000 * (i % 2), relabel)
            same(ix, m, MATCH_ALL, BY_LABEL, sums=bool(i % 2), what=f"{metric} {other}")
            same(ix, m, MATCH_ALL, BY_VALUE, 7, what=f"{metric} buckets of negative values")


def test_every_layout_at_the_bench_width(va):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((N, 768)).astype(np.float32)
    ix, m = make(va, rows, "bf16", "cosine", labels=np.zeros(N, np.uint32))
    with ix:
        for layout in LAYOUTS:
            labels = LAYOUTS[layout](N, rng)
            for h in (ix, m):
                h.set_labels(0, labels)
            wg, wv = same(ix, m, MATCH_ALL, BY_LABEL, what=layout)
            groups, vectors = ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL)    # the wrapper sizes itself
            assert groups.tobytes() == wg.tobytes() and vectors.tobytes() == wv.tobytes() and vectors.shape == (wg.size, 768)


def test_a_label_per_row_with_capacity_equal_to_the_groups(va):
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((N, 8)).astype(np.float32)
    labels = rng.permutation(N).astype(np.uint32) * np.uint32(2654435761)       # odd multiplier: distinct mod 2^32
    for dtype, metric in (("bf16", "l2"), ("f32", "cosine")):
        ix, m = make(va, rows, dtype, metric, off=1000, labels=labels)
        with ix:
            wg, wv, wr = m.centroids_where(MATCH_ALL, BY_LABEL)
            assert wg.size == N and (wg["count"] == 1).all()
            rc, n, n_rows, groups, vectors = raw_call(ix, MATCH_ALL, 0, BY_LABEL, 0, N)
            assert (rc, n, n_rows) == (0, N, N) and groups.tobytes() == wg.tobytes() and vectors.tobytes() == wv.tobytes()
            assert vectors.tobytes() == m.prepared()[np.argsort(labels, kind="stable")].tobytes()   # the mean of one row is the row
            rc, n, n_rows, groups, vectors = raw_call(ix, MATCH_ALL, 0, BY_LABEL, 0, N - 1)
            assert rc == ERR_CAPACITY and (n, n_rows) == (SENT, SENT) and untouched(groups, vectors)


# ---------------------------------------------------------------- keys
def test_keys_at_the_edges(va):
    rng = np.random.default_rng(13)
    rows = rng.standard_normal((N, 8)).astype(np.float32)
    labels = np.array([0, 0xFFFFFFFF, 1, 0x80000000], np.uint32)[rng.integers(0, 4, N)]
    values = np.array([I64_MIN, I64_MAX, -1, 0, -8, 6], np.int64)[rng.integers(0, 6, N)]
    ix, m = make(va, rows, "f32", "ip", off=1000, labels=labels, values=values)
    with ix:
        wg, _ = same(ix, m, MATCH_ALL, BY_LABEL)
        assert wg["key"].tolist() == [0, 1, 0x80000000, 0xFFFFFFFF]
        wg, _ = same(ix, m, MATCH_ALL, BY_VALUE, 1, sums=True)
        assert wg["key"].tolist() == [I64_MIN, -8, -1, 0, 6, I64_MAX]           # INT64_MIN, the table's marker, is a key like any other
        wg, _ = same(ix, m, MATCH_ALL, BY_VALUE, 7)
        assert -2 in wg["key"].tolist() and -1 in wg["key"].tolist()            # floor division: -8 // 7 == -2, -1 // 7 == -1
        same(ix, m, MATCH_ALL, BY_VALUE, I64_MAX)
    ix, m = make(va, rows[:300], "bf16", "cosine")                               # no column at all: one group with key 0
    with ix:
        for by, width in ((BY_LABEL, None), (BY_VALUE, 5)):
            wg, _ = same(ix, m, MATCH_ALL, by, width)
            assert wg.tolist() == [(0, 300, 0)]


# ---------------------------------------------------------------- rows considered
@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((N, 24)).astype(np.float32)
    values = rng.integers(-40, 40, N).astype(np.int64)
    tags = rng.integers(0, 16, N).astype(np.uint64) | (rng.integers(0, 2, N).astype(np.uint64) << np.uint64(63))
    labels = documents(N, rng) % np.uint32(50)
    allow = rng.random(N) < 0.8
    dead = np.unique(np.concatenate([rng.choice(np.arange(1, N), 200, replace=False), [0, 5, 2047, 2048, 4095, 4096, N - 1]])).astype(np.uint64)
    return rows, values, tags, labels, allow, dead


def restricted(va, world, dtype="bf16", metric="l2", off=1000):
    rows, values, tags, labels, allow, dead = world
    ix, m = make(va, rows, dtype, metric, off, labels, values, tags)
    for h in (m, ix):
        h.set_filter(allow)
        h.delete(dead + np.uint64(off))
    return ix, m


PREDS = [MATCH_ALL, (6, 1, 1 << 63, -30, 25, 0, 0), (1, 0, 0, *FULL, 0, 0), (0, 0, 8, -3, 20, 0, 0), (0, 0, 0, *FULL, 7, 1), (2, 1, 4, -39, 39, 11, 1)]


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_scope_predicate_and_id_offset(va, world, metric):
    ix, m = restricted(va, world, metric=metric)
    with ix:
        assert ix.count_where([MATCH_ALL], True)[0] < ix.count_where([MATCH_ALL])[0] < N   # both restrictions bite
        for pred in PREDS:
            for allowed in (False, True):
                wg, _ = same(ix, m, pred, BY_LABEL, allowed=allowed, what=str(pred))
                same(ix, m, pred, BY_VALUE, 7, sums=True, allowed=allowed, what=str(pred))
                assert wg.size and wg["first_id"].min() >= 1001                  # row 0 is deleted; ids carry the offset
        wg, _ = same(ix, m, PREDS[4], BY_LABEL)
        assert wg["key"].tolist() == [7]                                         # a predicate carrying a label: one group
        for pred in ((0, 1, 1, *FULL, 0, 0), (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1000, I64_MAX, 0, 0), (0, 0, 0, *FULL, 51, 1)):
            rc, n, rows, groups, vectors = raw_call(ix, pred, 0, BY_LABEL, 0, 4)   # unsatisfiable, or satisfiable with no row matching
            assert (rc, n, rows) == (0, 0, 0) and untouched(groups, vectors)
            same(ix, m, pred, BY_LABEL)


def test_after_update_and_compact(va, world):
    rng = np.random.default_rng(15)
    ix, m = restricted(va, world, dtype="f32", metric="ip")
    with ix:
        same(ix, m, MATCH_ALL, BY_LABEL, what="fresh")
        live = np.flatnonzero(~m.deleted)
        ids = (rng.choice(live, 300, replace=False) + 1000).astype(np.uint64)
        new = (rng.standard_normal((300, 24)) * 1000).astype(np.float32)
        for h in (ix, m):
            h.update(ids, new)
        same(ix, m, MATCH_ALL, BY_LABEL, what="after update")                    # the scale follows the new largest element
        gone = (np.flatnonzero(~m.deleted)[::5] + 1000).astype(np.uint64)
        for h in (ix, m):
            h.delete(gone)
            h.compact()
        assert ix.count == m.count < 4096                                        # fewer rows: R steps down with them
        same(ix, m, MATCH_ALL, BY_LABEL, sums=True, what="after compact")
        same(ix, m, MATCH_ALL, BY_VALUE, 7, allowed=True, what="after compact")


def test_an_empty_handle_gives_zero_groups(va):
    with va.Index(8, "f32", "l2") as ix:
        for reserve in (0, 500):
            if reserve:
                ix.reserve(reserve)
            for flags in (0, ALLOWED, CENTROID_SUM, ALLOWED | CENTROID_SUM):
                for by, width in ((BY_LABEL, 0), (BY_VALUE, 3)):
                    rc, n, rows, groups, vectors = raw_call(ix, MATCH_ALL, flags, by, width, 9)
                    assert (rc, n, rows) == (0, 0, 0) and untouched(groups, vectors)
            groups, vectors = ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL)
            assert groups.size == 0 and vectors.shape == (0, 8)


# ---------------------------------------------------------------- magnitudes (L2 and IP handles keep the values as given)
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_magnitudes_in_one_group(va, metric):
    rng = np.random.default_rng(16)
    n, dim = 4500, 12
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[0::5] *= np.float32(1e30)
    rows[1::5] *= np.float32(1e-30)
    rows[2::5] = (rng.integers(-(1 << 23) + 1, 1 << 23, (rows[2::5].shape)) * 2.0 ** -149).astype(np.float32)   # subnormals
    rows[3::5] = 0.0
    rows[3::5, ::2] = -0.0
    labels = rng.integers(0, 3, n).astype(np.uint32)
    ix, m = make(va, rows, "f32", metric, labels=labels)
    with ix:
        for sums in (False, True):
            same(ix, m, MATCH_ALL, BY_LABEL, sums=sums, what="1e30 and 1e-30 together")
        for h in (ix, m):
            h.delete(np.flatnonzero(np.arange(n) % 5 == 0).astype(np.uint64))    # without the large rows the scale drops by 200 binary orders
        for sums in (False, True):
            same(ix, m, MATCH_ALL, BY_LABEL, sums=sums, what="1e-30 and subnormals")
        for h in (ix, m):
            h.delete(np.flatnonzero(np.arange(n) % 5 == 1).astype(np.uint64))
            h.delete(np.flatnonzero(np.arange(n) % 5 == 4).astype(np.uint64))
        for sums in (False, True):
            _, wv = same(ix, m, MATCH_ALL, BY_LABEL, sums=sums, what="subnormals and zeros alone")
        assert (np.abs(wv) < 2.0 ** -100).all() and wv.any()
    x = rows[:600]
    ix, m = make(va, np.concatenate([x, -x]), "f32", metric, labels=np.concatenate([labels[:600], labels[:600]]))
    with ix:
        for sums in (False, True):
            _, wv = same(ix, m, MATCH_ALL, BY_LABEL, sums=sums, what="x and -x")
            assert (wv.view(np.uint32) == 0).all()                               # +0.0, never -0.0


@pytest.mark.parametrize("n", [4095, 4096])
def test_the_largest_value_in_every_row_at_the_step_of_r(va, n):
    """n rows of the largest fp32 in one group: |S| stays below 2^62 with nothing to spare at n = 2^R - 1.  The mean is
    the value itself, the sum overflows fp32 as the model's conversion does."""
    rows = np.full((n, 5), F32_MAX, np.float32)
    rows[:, 1] = -F32_MAX
    rows[:, 2] = np.float32(1.0)
    for metric in ("l2", "ip"):
        ix, m = make(va, rows, "f32", metric, labels=np.full(n, 9, np.uint32), reserve=0)
        with ix:
            with np.errstate(over="ignore"):
                _, wv = same(ix, m, MATCH_ALL, BY_LABEL, what=f"{n} rows")
                assert wv[0].tolist()[:2] == [F32_MAX, -F32_MAX]
                _, wv = same(ix, m, MATCH_ALL, BY_LABEL, sums=True, what=f"{n} rows")
                assert np.isinf(wv[0, 0]) and wv[0, 2] == 0                      # 1.0 lies 2^78 below this call's quantum
    rng = np.random.default_rng(n)                                               # and ordinary rows on both sides of the step
    rows = rng.standard_normal((n, 40)).astype(np.float32)
    ix, m = make(va, rows, "bf16", "cosine", labels=rng.integers(0, 5, n).astype(np.uint32), reserve=0)
    with ix:
        same(ix, m, MATCH_ALL, BY_LABEL, what=f"{n} rows, cosine")


def test_an_infinity_counts_only_in_a_considered_row(va):
    """A bf16 handle rounds the largest finite fp32 to an infinity, which get_rows reads back; add() accepts the row."""
    rng = np.random.default_rng(17)
    n = 4200
    rows = rng.standard_normal((n, 10)).astype(np.float32)
    rows[4100, 7] = F32_MAX
    labels = rng.integers(0, 4, n).astype(np.uint32)
    labels[4100] = 9
    ix, m = make(va, rows, "bf16", "l2", labels=labels)
    with ix:
        assert np.isinf(ix.get_rows(4100, 1)[0, 7]) and np.isinf(m.prepared()[4100, 7])
        for flags in (0, CENTROID_SUM):
            rc, cnt, n_rows, groups, vectors = raw_call(ix, MATCH_ALL, flags, BY_LABEL, 0, 8)
            assert rc == ERR_INVALID_ARG and (cnt, n_rows) == (SENT, SENT) and untouched(groups, vectors)
        with pytest.raises(ModelError):
            m.centroids_where(MATCH_ALL, BY_LABEL)
        with pytest.raises(va.VrodError) as e:
            ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL)
        assert e.value.code == ERR_INVALID_ARG
        same(ix, m, (0, 0, 0, *FULL, 2, 1), BY_LABEL, what="the row is not matched")
        for h in (ix, m):
            h.delete(np.array([4100], np.uint64))
        wg, _ = same(ix, m, MATCH_ALL, BY_LABEL, what="the row is deleted")
        assert wg.size == 4


# ---------------------------------------------------------------- determinism
def test_repeated_calls_and_permuted_rows_give_identical_bits(va):
    rng = np.random.default_rng(18)
    dim = 200
    rows = (rng.standard_normal((N, dim)) * np.exp(rng.uniform(-8, 8, (N, 1)))).astype(np.float32)
    labels = rng.integers(0, 7, N).astype(np.uint32)
    perm = rng.permutation(N)
    for dtype, metric in (("bf16", "cosine"), ("f32", "l2")):
        ix, m = make(va, rows, dtype, metric, labels=labels)
        jx, _ = make(va, rows[perm], dtype, metric, labels=labels[perm])
        with ix, jx:
            for sums in (False, True):
                wg, wv = same(ix, m, MATCH_ALL, BY_LABEL, sums=sums, what="determinism")
                for _ in range(3):
                    groups, vectors = ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL, sums=sums)
                    assert groups.tobytes() == wg.tobytes() and vectors.tobytes() == wv.tobytes()
                groups, vectors = jx.centroids_where(MATCH_ALL, va.AGG_BY_LABEL, sums=sums)
                assert np.array_equal(groups["key"], wg["key"]) and np.array_equal(groups["count"], wg["count"])
                assert vectors.tobytes() == wv.tobytes(), "the same rows in another order give other bits"


# ---------------------------------------------------------------- the device form
def test_the_device_form_gives_the_host_forms_bits(va):
    import torch
    rng = np.random.default_rng(19)
    for dim, dtype, metric in ((200, "bf16", "cosine"), (3, "f32", "l2")):
        rows = rng.standard_normal((N, dim)).astype(np.float32)
        ix, m = make(va, rows, dtype, metric, off=1000, labels=documents(N, rng) % np.uint32(300))
        with ix:
            wg, wv = same(ix, m, MATCH_ALL, BY_LABEL)
            big = torch.full((wg.size + 4, dim + 5), float("nan"), dtype=torch.float32, device="cuda")
            big.view(torch.int32).fill_(SENT32)
            groups, vectors = ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL, out=big[:, :dim])
            assert groups.tobytes() == wg.tobytes() and vectors.shape == (wg.size, dim) and vectors.data_ptr() == big.data_ptr()
            host = big.cpu().numpy().view(np.uint32)
            assert np.array_equal(host[:wg.size, :dim], wv.view(np.uint32)) and untouched(host[:, dim:], host[wg.size:])
            groups, vectors = ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL, sums=True, capacity=wg.size, out=None)
            dense = ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL, sums=True, capacity=wg.size,
                                       out=torch.empty((wg.size, dim), dtype=torch.float32, device="cuda"))[1]
            assert dense.cpu().numpy().tobytes() == vectors.tobytes()
            ids, _ = ix.search_device(big[:wg.size, :dim].contiguous(), 1)       # the centroids feed a search where they lie
            assert ids.shape == (wg.size, 1)


# ---------------------------------------------------------------- refusals
def test_refusals_write_nothing(va, world):
    import torch
    ix, m = restricted(va, world)
    rq = np.random.default_rng(20).standard_normal((2, 24)).astype(np.float32)
    with ix:
        ix.search(rq, K)
        before = ix.last_stats()
        bad = ix._row_preds(MATCH_ALL, 1).copy()
        bad["has_label"] = 2

        def refused(code, pred=MATCH_ALL, flags=0, by=BY_LABEL, width=0, capacity=64, stride=None, want=(True, True, True, True)):
            rc, n, rows, groups, vectors = raw_call(ix, pred, flags, by, width, capacity, room=64, stride=stride, want=want)
            assert rc == code and (n, rows) == (SENT, SENT) and untouched(groups, vectors)

        for flags in (2, 4, 16, 2 | ALLOWED, 0x80000000 | CENTROID_SUM):
            refused(ERR_INVALID_ARG, flags=flags)
        for by in (BY_TAG, 3, 0xFFFFFFFF):
            refused(ERR_INVALID_ARG, by=by)
        for width in (0, -1, I64_MIN):
            refused(ERR_INVALID_ARG, by=BY_VALUE, width=width)
        for capacity in (0, MAX_CENTROID_GROUPS + 1, 0xFFFFFFFF):
            refused(ERR_INVALID_ARG, capacity=capacity)
        refused(ERR_INVALID_ARG, stride=23)                                      # less than dim
        refused(ERR_INVALID_ARG, stride=0)
        refused(ERR_INVALID_ARG, stride=(1 << 64) // 64 + 1)                     # capacity * stride overflows
        refused(ERR_INVALID_ARG, pred=bad)
        refused(ERR_INVALID_ARG, pred=None)
        refused(ERR_INVALID_ARG, want=(False, True, True, True))                 # null out_count
        refused(ERR_INVALID_ARG, want=(True, True, False, True))                 # null out_groups
        refused(ERR_INVALID_ARG, want=(True, True, True, False))                 # null vectors
        assert raw_call(ix, MATCH_ALL, 0, BY_LABEL, -1, 64, want=(True, False, True, True))[:2] == (0, 50)   # width unread, out_rows optional
        for capacity in (1, 49):                                                 # 50 groups
            refused(ERR_CAPACITY, capacity=capacity)
        with pytest.raises(va.VrodError) as e:
            ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL, capacity=49)
        assert e.value.code == ERR_CAPACITY
        si = torch.empty((4, K), dtype=torch.int64, device="cuda")
        ss = torch.empty((4, K), dtype=torch.float32, device="cuda")
        ix.search_begin_synthetic_device(2, 0, 4, K, si, ss)                     # a pending search
        refused(ERR_INVALID_ARG)
        with pytest.raises(va.VrodError) as e:
            ix.centroids_where(MATCH_ALL, va.AGG_BY_LABEL)
        assert e.value.code == ERR_INVALID_ARG
        ix.search_end()
        ix.search(rq, K)
        assert ix.last_stats() == before                                         # the same search, the same counters
        same(ix, m, MATCH_ALL, BY_LABEL, what="after the refused calls")
        assert ix.last_stats() == before


def test_a_multi_device_handle_is_unsupported(va):
    rows = np.random.default_rng(21).standard_normal((500, 8)).astype(np.float32)
    with va.Index(8, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(rows)
        for by, width in ((BY_LABEL, 0), (BY_VALUE, 3)):
            rc, n, n_rows, groups, vectors = raw_call(ix, MATCH_ALL, CENTROID_SUM, by, width, 4)
            assert rc == ERR_UNSUPPORTED and (n, n_rows) == (SENT, SENT) and untouched(groups, vectors)
        assert (ix.count, ix.live_count()) == (500, 500)
