"""The oracle's range function (oracle/vrod_oracle.c orc_scan_range, oracle.scan_range / range_search) pinned on the CPU:
against the composition tests/test_gpu_range.py used before it existed (top-k with k = all eligible rows, then the
qualifying prefix), against a numpy restatement (numpy_scores_canonical + a comparison + a lexsort), and on the rules of
include/vrod.h: inclusive boundary, a NaN score never qualifies, best first then id.  No GPU."""
import numpy as np
import pytest

from support import DT, assert_same_all_bits, bits, prep_of, form_of

METRICS = ["cosine", "l2", "ip"]


def assert_same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"{what}: lims {got[0][:8]} != {want[0][:8]}"
    assert got[1].dtype == np.uint64 and got[2].dtype == np.float32
    assert_same_all_bits(got[1], got[2], want[1], want[2], what)


def prefix_composition(O, raw, rq, thr, dtype, metric, elig=None, id_offset=0):
    """What test_gpu_range.py computed: scan_topk over the eligible rows with k = all of them, ids mapped through
    elig, the qualifying prefix of every row."""
    elig = np.arange(raw.shape[0]) if elig is None else np.asarray(elig)
    pc = O.prepare(np.ascontiguousarray(raw[elig]), DT[dtype], prep_of(metric))
    pq = O.prepare(rq, DT[dtype], prep_of(metric))
    ids, sc = O.scan_topk(pc, pq, elig.size, form_of(metric), threads=3)
    ids = elig.astype(np.uint64)[ids.astype(np.int64)]
    lims, oi, osc = [0], [], []
    with np.errstate(invalid="ignore"):
        for q in range(rq.shape[0]):
            ok = (sc[q] <= np.float32(thr[q])) if metric == "l2" else (sc[q] >= np.float32(thr[q]))
            n = int(ok.sum())
            assert ok[:n].all()
            oi.append(ids[q, :n] + np.uint64(id_offset))
            osc.append(sc[q, :n])
            lims.append(lims[-1] + n)
    return np.array(lims, np.uint64), np.concatenate(oi), np.concatenate(osc)


def thresholds_from(S, metric):
    """Per query, cycling: exactly the 1st / 10th / 300th best score, a midpoint, better than the best."""
    srt = np.sort(S, axis=1)
    if metric != "l2":
        srt = srt[:, ::-1]
    thr = np.empty(S.shape[0], np.float32)
    for q in range(S.shape[0]):
        kind = q % 5
        if kind < 3:
            thr[q] = srt[q, (0, 9, 299)[kind]]
        elif kind == 3:
            thr[q] = np.float32((np.float64(srt[q, 20]) + np.float64(srt[q, 21])) / 2)
        else:
            thr[q] = np.nextafter(srt[q, 0], np.float32(np.inf if metric != "l2" else -np.inf))
    return thr


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_equals_the_prefix_composition_and_numpy(oracle, dtype, metric, masked):
    rng = np.random.default_rng(31)
    n, dim, nq = 1500, 40, 11
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    raw[700:712] = raw[3]                                   # tied scores: the order among them is by id
    rq = rng.standard_normal((nq, dim)).astype(np.float32)
    mask = rng.random(n) < 0.6 if masked else None
    if masked:
        mask[3] = mask[705] = True
    off = 1000 if masked else 0
    pc = oracle.prepare(raw, DT[dtype], prep_of(metric))
    pq = oracle.prepare(rq, DT[dtype], prep_of(metric))
    S = oracle.numpy_scores_canonical(pc, pq, form_of(metric))
    thr = thresholds_from(S[:, mask] if masked else S, metric)
    thr[1] = S[1, 705]                                       # the tied rows exactly at a threshold
    got = oracle.scan_range(pc, pq, thr, form_of(metric), mask=mask, id_offset=off, threads=1)
    elig = np.flatnonzero(mask) if masked else None
    assert_same(got, prefix_composition(oracle, raw, rq, thr, dtype, metric, elig, off), "prefix")
    assert_same(got, oracle.numpy_range_from_scores(S, thr, form_of(metric), mask, off), "numpy")
    assert_same(got, oracle.range_search(raw, rq, thr, DT[dtype], prep_of(metric), form_of(metric), mask, off, threads=4), "end to end")
    counts = np.diff(got[0].astype(np.int64))
    assert counts[0] == 1 and counts[4] == 0 and counts[3] == 21 and counts[2] == 300, counts
    seg = got[1][int(got[0][1]):int(got[0][2])] - np.uint64(off)
    tied = [r for r in [3] + list(range(700, 712)) if mask is None or mask[r]]
    assert seg[-len(tied):].tolist() == tied                 # inclusive, and in id order


@pytest.mark.parametrize("metric", METRICS)
def test_threaded_equals_single_threaded(oracle, metric):
    rng = np.random.default_rng(32)
    raw = rng.standard_normal((5003, 24)).astype(np.float32)
    raw[::7] = raw[0]
    rq = rng.standard_normal((9, 24)).astype(np.float32)
    pc = oracle.prepare(raw, 1, prep_of(metric))
    pq = oracle.prepare(rq, 1, prep_of(metric))
    S = oracle.numpy_scores_canonical(pc, pq, form_of(metric))
    thr = np.sort(S, axis=1)[:, 5003 // 2].astype(np.float32)     # about half of the rows each, the copies included
    thr[0] = S[0, 0]
    mask = rng.random(5003) < 0.9
    one = oracle.scan_range(pc, pq, thr, form_of(metric), mask=mask, id_offset=7, threads=1)
    assert int(one[0][-1]) > 9 * 2000
    for t in (2, 3, 16, 6000):
        assert_same(oracle.scan_range(pc, pq, thr, form_of(metric), mask=mask, id_offset=7, threads=t), one, f"threads={t}")


@pytest.mark.parametrize("metric", METRICS)
def test_infinite_thresholds(oracle, metric):
    rng = np.random.default_rng(33)
    raw = rng.standard_normal((300, 16)).astype(np.float32)
    rq = rng.standard_normal((4, 16)).astype(np.float32)
    open_, shut = (np.inf, -np.inf) if metric == "l2" else (-np.inf, np.inf)
    thr = np.array([open_, shut, open_, shut], np.float32)
    lims, ids, sc = oracle.range_search(raw, rq, thr, 0, prep_of(metric), form_of(metric), threads=2)
    assert np.diff(lims.astype(np.int64)).tolist() == [300, 0, 300, 0]
    ti, ts = oracle.scan_topk(oracle.prepare(raw, 0, prep_of(metric)), oracle.prepare(rq, 0, prep_of(metric)), 300, form_of(metric))
    assert np.array_equal(ids[:300], ti[0]) and np.array_equal(bits(sc[:300]), bits(ts[0]))
    assert np.array_equal(ids[300:], ti[2]) and np.array_equal(bits(sc[300:]), bits(ts[2]))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_duplicated_row_exactly_at_the_threshold(oracle, dtype, metric):
    rng = np.random.default_rng(34)
    base = rng.standard_normal((900, 32)).astype(np.float32)
    raw = np.concatenate([base[:400], np.repeat(base[7:8], 50, axis=0), base[400:]])
    rq = (base[7:8] + 0.5 * rng.standard_normal((1, 32))).astype(np.float32)
    pc = oracle.prepare(raw, DT[dtype], prep_of(metric))
    pq = oracle.prepare(rq, DT[dtype], prep_of(metric))
    t = oracle.numpy_scores_canonical(pc, pq, form_of(metric))[0, 7]
    worse = np.float32(np.inf if metric == "l2" else -np.inf)
    at = oracle.scan_range(pc, pq, t, form_of(metric), threads=3)
    looser = oracle.scan_range(pc, pq, np.nextafter(t, worse), form_of(metric), threads=3)
    tighter = oracle.scan_range(pc, pq, np.nextafter(t, -worse), form_of(metric), threads=3)
    copies = [7] + list(range(400, 450))
    assert at[1][-51:].tolist() == copies and (bits(at[2][-51:]) == bits(t)).all()
    assert_same(looser, at, "one float looser: the same rows")
    assert int(tighter[0][1]) == int(at[0][1]) - 51 and np.array_equal(tighter[1], at[1][:-51])


def test_ip_with_infinite_and_nan_scores(oracle):
    rng = np.random.default_rng(35)
    n, d = 400, 8
    raw = rng.standard_normal((n, d)).astype(np.float32)
    raw[10:20, 0] = 1e20                                       # q0 . x = +inf
    raw[20:30, 0] = -1e20                                      # -inf
    raw[30:40, 0], raw[30:40, 1] = 1e20, -1e20                 # inf - inf = NaN
    q0 = np.ones(d, np.float32)
    q0[:2] = 1e20
    rq = np.stack([q0, q0, q0, q0, rng.standard_normal(d).astype(np.float32)])
    S = oracle.numpy_scores_canonical(raw, rq, 0)
    assert np.isnan(S[0, 30:40]).all() and np.isposinf(S[0, 10:20]).all() and np.isneginf(S[0, 20:30]).all()
    thr = np.array([-np.inf, np.inf, 0.0, -3.4e38, S[4, 5]], np.float32)
    got = oracle.range_search(raw, rq, thr, 0, 1, 0, threads=3)
    assert_same(got, oracle.numpy_range_from_scores(S, thr, 0), "numpy")
    counts = np.diff(got[0].astype(np.int64)).tolist()
    assert counts[0] == n - 10                                # every row but the NaN-scored ones, the -inf ones included
    assert counts[1] == 10 and got[1][n - 10:n].tolist() == list(range(10, 20))    # +inf >= +inf
    assert counts[3] == n - 20                                # the -inf rows drop out below any finite threshold
    assert not np.isnan(got[2]).any()
    assert got[1][:10].tolist() == list(range(10, 20)) and got[1][n - 20:n - 10].tolist() == list(range(20, 30))


def test_empty_corpus_and_no_queries_and_bad_arguments(oracle):
    q = np.ones((3, 8), np.float32)
    lims, ids, sc = oracle.scan_range(np.zeros((0, 8), np.float32), q, 0.5, 0, threads=4)
    assert lims.tolist() == [0, 0, 0, 0] and ids.size == 0 and sc.size == 0 and ids.dtype == np.uint64
    lims, ids, sc = oracle.range_search(np.zeros((0, 8), np.float32), q, [0.0, 1.0, 2.0], 1, 0, 0)
    assert lims.tolist() == [0, 0, 0, 0]
    c = np.ones((5, 8), np.float32)
    lims, ids, sc = oracle.scan_range(c, q[:0], np.zeros(0, np.float32), 1, threads=2)
    assert lims.tolist() == [0] and ids.size == 0
    lims, ids, sc = oracle.scan_range(c, q, 0.0, 1, mask=np.zeros(5, bool))
    assert lims.tolist() == [0, 0, 0, 0]
    lims, ids, sc = oracle.scan_range(c, q, 0.0, 1, id_offset=2 ** 40)          # identical rows at distance 0
    assert ids.tolist() == [2 ** 40 + r for r in range(5)] * 3
    with pytest.raises(RuntimeError):
        oracle.scan_range(c, q, np.nan, 0)
    with pytest.raises(RuntimeError):
        oracle.scan_range(c, q, 0.0, 2)
    with pytest.raises(ValueError):
        oracle.scan_range(c, q, 0.0, 0, mask=np.ones(4, bool))
    with pytest.raises(ValueError):
        oracle.scan_range(c, np.ones((3, 7), np.float32), 0.0, 0)       # dims differ: never reaches C
    with pytest.raises(ValueError):
        oracle.scan_range(c, q, [0.0, 1.0], 0)


def test_merge_over_row_blocks_equals_one_scan(oracle):
    rng = np.random.default_rng(36)
    raw = rng.standard_normal((4000, 16)).astype(np.float32)
    raw[[5, 1500, 1501, 3999]] = raw[0]
    rq = np.concatenate([raw[:1], rng.standard_normal((5, 16)).astype(np.float32)])
    for form in (0, 1):
        S = oracle.numpy_scores_canonical(raw, rq, form)
        thr = np.sort(S, axis=1)[:, 2000].astype(np.float32)
        thr[0] = S[0, 0]
        whole = oracle.scan_range(raw, rq, thr, form, threads=2)
        parts = [oracle.scan_range(raw[lo:hi], rq, thr, form, id_offset=lo, threads=2) for lo, hi in ((0, 1501), (1501, 1501), (1501, 4000))]
        assert_same(oracle.merge_range(parts, form), whole, f"form {form}")
