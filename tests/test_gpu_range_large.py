"""Range searches at the sizes where the batched kernels reach their steady state, against the oracle's range function.

tests/test_gpu_range.py runs the 4-wave kernel at 5000 rows only.  Here: 1.3M rows (strips of 54-55 tiles with an odd
stealing tail, tests/test_gpu_steal.py) with thresholds that list tens, thousands, more than a list (8192: the row
range is redone in pieces) and no rows, with stealing on and off; thresholds that qualify a quarter, half and all of
the rows of every query at once under a deleted stripe and a dense allow-list; more than 2^24 rows (two launches before
any split); the K-tile counts tests/test_gpu_parity.py insists on; and the result sort (kernels_range.hip: 2048-entry
chunks, then merge passes between two buffers) from 2049 to more than 3 000 000 entries, with an odd and an even number
of passes, a segment of more than a million entries, thousands of entries tied on (query, score), and two shards.
The reference is oracle.range_search; a corpus too large for one call is scanned in row blocks and merged."""
import os
import subprocess
import sys

import numpy as np
import pytest

from support import DT, PATH_MFMA, THREADS, va, bits, assert_same_all_bits, prep_of, form_of, hard_thresholds  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST_CAP = 8192                      # entries of a query's hit list (kSelectChunk)
SORT_CHUNK = 2048                    # kernels_range.hip kRangeSortChunk


def worse(metric):
    return np.float32(np.inf if metric == "l2" else -np.inf)


def assert_range(got, want, what):
    (lims, ids, sc), (ol, oi, osc) = got, want
    assert np.array_equal(lims, ol), f"{what}: counts differ at queries {np.argwhere(np.diff(lims.astype(np.int64)) != np.diff(ol.astype(np.int64)))[:8].ravel()}"
    assert_same_all_bits(ids, sc, oi, osc, what)


def reference(O, raw, rq, thr, dtype, metric, mask=None, block=4_000_000):
    """oracle.range_search, over row blocks when the corpus is large (a range answer is a union over row blocks)."""
    n = raw.shape[0]
    if n <= block:
        return O.range_search(raw, rq, thr, DT[dtype], prep_of(metric), form_of(metric), mask=mask, threads=THREADS)
    parts = [O.range_search(raw[lo:lo + block], rq, thr, DT[dtype], prep_of(metric), form_of(metric),
                            mask=None if mask is None else mask[lo:lo + block], id_offset=lo, threads=THREADS) for lo in range(0, n, block)]
    return O.merge_range(parts, form_of(metric))


def sorted_scores(O, raw, rq, dtype, metric, mask=None):
    """[nq, m] canonical scores of the (eligible) rows, best first."""
    lims, _, sc = O.range_search(raw, rq, worse(metric), DT[dtype], prep_of(metric), form_of(metric), mask=mask, threads=THREADS)
    m = int(lims[1])
    assert np.array_equal(lims, np.arange(rq.shape[0] + 1, dtype=np.uint64) * np.uint64(m))
    return sc.reshape(rq.shape[0], m)


def merge_passes(total):
    """As launch_range_sort: runs of 2048 doubled until one covers everything."""
    passes, run = 0, SORT_CHUNK
    while run < total:
        passes, run = passes + 1, run * 2
    return passes


def show(what, st, got):
    print(what, {k: st[k] for k in ("path", "split_pass", "kprime", "scan_launches", "fallback_queries", "max_fast_err", "eps_bound")},
          "total", int(got[0][-1]), "passes", merge_passes(int(got[0][-1])))


def check_fast(st, what, split):
    assert st["path"] == PATH_MFMA and st["fallback_queries"] == 0 and st["split_pass"] == (1 if split == "1" else 0), (what, st)
    assert np.isfinite(st["eps_bound"]) and st["max_fast_err"] <= st["eps_bound"], (what, st)


# ---------------------------------------------------------------- 1.3M rows: steady state, stealing, split-and-redo
N_STEADY, DIM_STEADY = 1_300_000, 128
DUP_ROWS = (255, 256, 257, 65535, 65536, 700_001, 1_299_999)       # copies of row 5: across tile, block and strip ends
FORMS_STEADY = [("bf16", None), ("f32", "1")]


def steady_inputs(O):
    """The synthetic stream with row norms spread over 0.5 .. 2 (so that IP is not cosine) and the planted copies; 300
    queries, query 0 near the copied row."""
    rng = np.random.default_rng(77)
    raw = O.synth_rows(61, 0, N_STEADY, DIM_STEADY, threads=THREADS)
    raw *= rng.uniform(0.5, 2.0, (N_STEADY, 1)).astype(np.float32)
    for r in DUP_ROWS:
        raw[r] = raw[5]
    rq = O.synth_rows(62, 0, 300, DIM_STEADY) * rng.uniform(0.5, 2.0, (300, 1)).astype(np.float32)
    rq[0] = raw[5] + 0.05 * rq[0]
    return raw, np.ascontiguousarray(rq, dtype=np.float32)


def steady_thresholds(O, raw, rq, dtype, metric):
    """From the scores of the first 65 000 rows (1 / 20 of the corpus), per query cycling: tens of rows (sample rank 2),
    thousands (rank 150 -> ~3000); query 1 more than a list (rank 600 -> ~12 000), query 2 nothing -- a finite
    threshold one float better than its best score over the whole corpus, so that the kernel's compare runs --, query 0
    exactly the planted copies' score."""
    s = sorted_scores(O, raw[:65000], rq, dtype, metric)
    thr = np.where(np.arange(rq.shape[0]) % 8 == 7, s[:, 150], s[:, 2]).astype(np.float32)
    thr[1] = s[1, 600]
    thr[2] = np.nextafter(sorted_scores(O, raw, rq[2:3], dtype, metric)[0, 0], -worse(metric))
    pc = O.prepare(raw[5:6], DT[dtype], prep_of(metric))
    pq = O.prepare(rq[:1], DT[dtype], prep_of(metric))
    thr[0] = O.numpy_scores_canonical(pc, pq, form_of(metric))[0, 0]
    return thr


class TestSteadyState:
    """The 1.3M-row corpus lives for this class only: it is released before the later, larger cases run."""

    @pytest.fixture(scope="class")
    def steady(self, oracle):
        yield steady_inputs(oracle)

    @pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
    @pytest.mark.parametrize("dtype, split", FORMS_STEADY)
    def test_steady_state_with_mixed_thresholds(self, va, oracle, steady, dtype, split, metric):
        from conftest import f32_split
        raw, rq_all = steady
        with f32_split(split), va.Index(DIM_STEADY, dtype, metric) as ix:
            ix.add(raw)
            ix.set_path(PATH_MFMA)
            for nq in ((100, 300) if dtype == "bf16" else (100,)):
                rq = rq_all[:nq]
                thr = steady_thresholds(oracle, raw, rq, dtype, metric)
                got = ix.range_search(rq, thr)
                st = ix.last_stats()
                what = f"steady {dtype}/{split}/{metric}/{nq}"
                show(what, st, got)
                want = reference(oracle, raw, rq, thr, dtype, metric)
                assert_range(got, want, what)
                check_fast(st, what, split)
                counts = np.diff(want[0].astype(np.int64))
                assert counts[1] > LIST_CAP and st["scan_launches"] > 1, (what, counts[:8], st)     # redone in pieces
                assert counts[2] == 0 and np.isfinite(thr[2]) and counts[0] >= len(DUP_ROWS) + 1
                assert np.median(counts) < 500 and (counts[7::8] >= 1000).all(), counts[:16]
                seg0 = got[1][:int(got[0][1])].tolist()
                assert seg0[-(len(DUP_ROWS) + 1):] == [5] + list(DUP_ROWS), seg0[-10:]


_STEAL_CODE = r'''
import sys, numpy as np
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import vrod_amd as va
from oracle import oracle as O
import test_gpu_range_large as T
raw, rq = T.steady_inputs(O)
thr = T.steady_thresholds(O, raw, rq, "bf16", "cosine")
with va.Index(T.DIM_STEADY, "bf16", "cosine") as ix:
    ix.add(raw); ix.set_path(2)
    lims, ids, sc = ix.range_search(rq, thr)
np.savez(sys.argv[1], lims=lims, ids=ids, sc=sc.view(np.uint32))
'''


def test_stealing_off_gives_the_same_bits(oracle):
    """As tests/test_gpu_steal.py does for top-k: the 300-query search over 1.3M rows in two processes,
    VROD_DEBUG_W4_STEAL=1 and 0."""
    outs = []
    for mode in ("1", "0"):
        path = f"/tmp/vrod_range_steal_{os.getpid()}_{mode}.npz"
        env = dict(os.environ, VROD_DEBUG_W4_STEAL=mode)
        env.pop("VROD_F32_SPLIT", None)
        r = subprocess.run([sys.executable, "-c", _STEAL_CODE, path], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(path) as z:
            outs.append((z["lims"], z["ids"], z["sc"]))
        os.unlink(path)
    assert int(outs[0][0][-1]) > 20000
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- dense hits under a deleted stripe and an allow-list
@pytest.mark.parametrize("dtype, split, metric", [("bf16", None, "cosine"), ("bf16", None, "l2"), ("bf16", None, "ip"), ("f32", "1", "l2")])
def test_dense_hits_with_deletes_and_a_filter(va, oracle, dtype, split, metric):
    """100 queries that each qualify a quarter, half and all of the eligible rows: every tile dumps a large share of its
    accumulators, every list overflows and the rows are redone in pieces."""
    from conftest import f32_split
    rng = np.random.default_rng(81)
    n, dim, nq = 50_000, 128, 100
    raw = (oracle.synth_rows(63, 0, n, dim, threads=THREADS) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    rq = (oracle.synth_rows(64, 0, nq, dim) * rng.uniform(0.5, 2.0, (nq, 1))).astype(np.float32)
    allow = rng.random(n) < 0.8
    stripe = np.arange(20_000, 23_000)                  # whole tiles and two partial ones
    mask = allow.copy()
    mask[stripe] = False
    m = int(mask.sum())
    s = sorted_scores(oracle, raw, rq, dtype, metric, mask)
    assert s.shape == (nq, m)
    with f32_split(split), va.Index(dim, dtype, metric) as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        ix.delete(stripe)
        ix.set_filter(allow)
        for share in (0.25, 0.5, 1.0):
            thr = np.full(nq, worse(metric), np.float32) if share == 1.0 else s[:, int(m * share) - 1].copy()
            got = ix.range_search(rq, thr)
            st = ix.last_stats()
            what = f"dense {dtype}/{split}/{metric}/{share}"
            show(what, st, got)
            assert_range(got, reference(oracle, raw, rq, thr, dtype, metric, mask), what)
            check_fast(st, what, split)
            counts = np.diff(got[0].astype(np.int64))
            if share == 1.0:
                assert (counts == m).all(), counts[:8]      # exactly the eligible rows
            else:
                assert (counts >= int(m * share)).all() and (counts <= int(m * share) + 8).all(), counts[:8]
            assert st["scan_launches"] > 1, (what, st)


# ---------------------------------------------------------------- more than 2^24 rows
@pytest.mark.parametrize("nq, metric", [(12, "cosine"), (100, "l2")], ids=["skinny-cosine", "w4-l2"])
def test_past_2pow24_rows(va, oracle, nq, metric):
    """Rows are addressed relative to a launch's first tile with 24 bits: the corpus of
    test_mfma_path_splits_launches_past_2pow24_rows at a small dim.  Copies of row 5 just below and above row 2^24, in
    the last full tile (n - 200) and in the last, partial tile of 97 rows (n - 50, n - 1); query 0 asks for exactly
    their score.  Then query 1 loosened to more than a list: its
    pieces' bounds are not the launch cut."""
    n, dim = (1 << 24) + 2_300_001, 16
    cut = 1 << 24
    dups = (cut - 1, cut, cut + 1, n - 200, n - 50, n - 1)
    assert n % 256 == 97
    raw = oracle.synth_rows(65, 0, n, dim, threads=THREADS)
    for r in dups:
        raw[r] = raw[5]
    rq = oracle.synth_rows(66, 0, nq, dim)
    rq[0] = raw[5] + 0.05 * rq[0]
    s = sorted_scores(oracle, raw[:1_000_000], rq, "bf16", metric)
    tight = s[:, 3].copy()                                # ~60 rows of 19M
    pq = oracle.prepare(rq[:1], 1, prep_of(metric))
    tight[0] = oracle.numpy_scores_canonical(oracle.prepare(raw[5:6], 1, prep_of(metric)), pq, form_of(metric))[0, 0]
    loose = tight.copy()
    loose[1] = s[1, 1600]                                 # ~30 000 rows
    with va.Index(dim, "bf16", metric) as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        got_t = ix.range_search(rq, tight)
        st_t = ix.last_stats()
        got_l = ix.range_search(rq, loose)
        st_l = ix.last_stats()
    show(f"2^24 tight {nq}/{metric}", st_t, got_t)
    show(f"2^24 loose {nq}/{metric}", st_l, got_l)
    want_t = reference(oracle, raw, rq, tight, "bf16", metric)
    want_l = reference(oracle, raw, rq, loose, "bf16", metric)
    del raw
    assert_range(got_t, want_t, "tight")
    assert_range(got_l, want_l, "loose")
    check_fast(st_t, "tight", None)
    check_fast(st_l, "loose", None)
    seg0 = got_t[1][:int(got_t[0][1])].tolist()
    assert seg0[-7:] == [5] + list(dups), seg0[-9:]
    assert int(np.diff(want_t[0].astype(np.int64)).max()) < LIST_CAP // 2 and st_t["scan_launches"] >= 2, st_t   # the 2^24 cut alone
    assert int(want_l[0][2] - want_l[0][1]) > LIST_CAP and st_l["scan_launches"] > st_t["scan_launches"], st_l


# ---------------------------------------------------------------- K-tile counts
def skinny_max_queries(dim, split):
    """kernels_mfma_skinny.hip mfma_skinny_max_queries restated: the queries' K extent (bf16 rows: dim rounded up to 64,
    2 bytes; the [hi | lo] planes: twice that) must fit in 160 KiB of LDS next to the hit logs (8 waves x 256 x 8 B),
    64 / 32 queries (bf16 rows) or 32 / 16 (planes) at a time.  A batch of at most that many queries runs the skinny
    kernel, a larger one the 4-wave kernel."""
    row_bytes = (dim + 63) // 64 * 64 * 2 * (2 if split else 1)
    fits = lambda nt: nt * 16 * (row_bytes + 32) + 8 * 256 * 8 <= 160 * 1024
    if split:
        return 32 if fits(2) else 16 if fits(1) else 0
    return 64 if fits(4) else 32 if fits(2) else 0


K_DIMS = [(40, "cosine"), (129, "l2"), (300, "ip"), (768, "l2"), (4096, "cosine")]
# (kernel, dtype, VROD_F32_SPLIT, queries, dim, metric).  No batch of 4096-d queries fits the skinny kernel's LDS: its
# long row is 2048 elements, 32 queries at a time (33 would take the 4-wave kernel).
KERNEL_FORMS = [(k, dt, sp, nq, dim, me) for k, dt, sp, nq in (("w4", "bf16", None, 100), ("w4-split", "f32", "1", 100), ("phased", "f32", "0", 100))
                for dim, me in K_DIMS] + [("skinny", "bf16", None, 33, dim, me) for dim, me in K_DIMS[:4]] + [("skinny", "bf16", None, 32, 2048, "cosine")]


@pytest.mark.parametrize("kernel, dtype, split, nq, dim, metric", KERNEL_FORMS, ids=[f"{k[0]}-{k[4]}-{k[5]}" for k in KERNEL_FORMS])
def test_k_tile_counts(va, oracle, kernel, dtype, split, nq, dim, metric):
    """One K-tile with a remainder, 3 (odd, one element over), 5, 12 and a long row, on every batched kernel.  Which
    kernel a batch reaches follows from the dispatcher's rule, restated in skinny_max_queries and checked here."""
    if kernel == "skinny":
        assert 4 < nq <= skinny_max_queries(dim, False)
    elif kernel == "w4":
        assert nq > skinny_max_queries(dim, False)
    elif kernel == "w4-split":
        assert nq > skinny_max_queries(dim, True)
    from conftest import f32_split
    rng = np.random.default_rng(dim)
    n = 20_000
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((nq, dim)).astype(np.float32)
    thr = hard_thresholds(sorted_scores(oracle, raw, rq, dtype, metric), metric)
    with f32_split(split), va.Index(dim, dtype, metric) as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        got = ix.range_search(rq, thr)
        st = ix.last_stats()
    what = f"ktiles {kernel} d={dim} {metric}"
    show(what, st, got)
    assert_range(got, reference(oracle, raw, rq, thr, dtype, metric), what)
    check_fast(st, what, split)
    counts = np.diff(got[0].astype(np.int64))
    assert counts[0] >= 1 and counts[1] >= 10 and counts[2] >= 1000 and counts[3] == 21 and counts[4] == 0, counts[:5]


# ---------------------------------------------------------------- the result sort
def test_sort_sizes_ties_and_pass_parities(va, oracle):
    """Totals of 2049, 4096 and 4097 entries (a second chunk of one entry, two full chunks, a third run of one entry
    whose sibling is absent), ~100 000, a single segment of 1.2M and 300 segments of 10 000+ (3M+), 5000 of them tied on
    (query, score): copies of one row spread over the whole corpus, ordered by id alone across chunks and runs.  The
    number of merge passes decides which buffer holds the result: both parities must occur."""
    rng = np.random.default_rng(91)
    dim = 16
    parities = set()
    big = oracle.synth_rows(67, 0, 1_200_000, dim, threads=THREADS)
    copies = np.arange(3, 140_000, 28)                     # 5000 rows, on both shards of the two-shard handle
    big[copies] = big[3]
    q300 = oracle.synth_rows(68, 0, 300, dim)
    q300[0] = big[3] + 0.05 * q300[0]

    def run(raw, rq, thr, metric, what, devices=None):
        kw = {} if devices is None else {"devices": devices}
        with va.Index(dim, "bf16", metric, **kw) as ix:
            ix.add(raw)
            ix.set_path(PATH_MFMA)
            got = ix.range_search(rq, thr)
            st = ix.last_stats()
        show(what, st, got)
        assert_range(got, reference(oracle, raw, rq, thr, "bf16", metric), what)
        assert st["path"] == PATH_MFMA and st["fallback_queries"] == 0, (what, st)
        parities.add(merge_passes(int(got[0][-1])) % 2)
        return got

    # every row of every query: exact totals
    for rows, nq, metric in ((683, 3, "cosine"), (1024, 4, "l2"), (241, 17, "ip"), (1000, 100, "cosine")):
        got = run(big[100_000:100_000 + rows], q300[1:1 + nq], np.full(nq, worse(metric), np.float32), metric, f"sort {rows}x{nq}")
        assert int(got[0][-1]) == rows * nq
    assert {merge_passes(t) for t in (2049, 4096, 4097, 100_000)} == {1, 2, 6}

    # one segment longer than a million entries among short ones
    rq = q300[1:8]
    s = sorted_scores(oracle, big[:100_000], rq, "bf16", "l2")
    thr = s[:, 5].copy()
    thr[3] = np.inf
    got = run(big, rq, thr, "l2", "sort one long segment")
    assert int(got[0][4] - got[0][3]) == 1_200_000

    # 300 segments of 10 000+ entries; query 0's boundary is the score of the 5000 copies
    raw = big[:140_000]                                    # blocks of 65536 rows: two on shard 0, one on shard 1
    s = sorted_scores(oracle, raw, q300, "bf16", "cosine")
    thr = s[:, 10_100].copy()
    thr[0] = s[0, 0]
    assert (bits(s[0, :5000]) == bits(s[0, 0])).all() and s[0, 5000] < s[0, 0], "the copies are query 0's best rows, tied"
    got = run(raw, q300, thr, "cosine", "sort 3M")
    assert int(got[0][-1]) >= 3_000_000 and merge_passes(int(got[0][-1])) == 11
    assert got[1][:5000].tolist() == copies.tolist()        # the tied entries: by id alone
    two = run(raw, q300, thr, "cosine", "sort 3M two shards", devices=[0, 0])
    assert_range(two, got, "two shards = one")
    assert parities == {0, 1}, parities
