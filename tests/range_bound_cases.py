"""Inputs of tests/test_gpu_range_bound.py: range searches on the bound-reaching families of certificate_fixtures.py,
with thresholds placed where the fast pass's error can matter.  Everything here runs on the CPU (numpy + the oracle):
tests/test_range_bound_cases.py checks every case without a device, the GPU test runs the same cases on the library.

A range search keeps only the rows whose FAST score is inside the caller's threshold widened by the error bound
(search_plan.h range_fast_threshold); a row outside is never seen again.  So a case tests that premise only if rows
lie within one bound of the threshold, on both sides of it.  Per query the threshold is the canonical score of the row
at the densest place of that query's score distribution (the rank with the most rows within one bound of it; on
near_ties: a member of the query's cluster, at a score level that leaves members on both sides), then -- cycling
over the queries -- exactly that score (the inclusive boundary), one float to the worse side (the same rows), one
float to the better side (that row and its ties drop out).
The bound is certificate_fixtures.mfma_eps, the Python restatement, for the batch's largest |q| and the corpus's largest
|x| as the library forms it -- not the eps_bound a search reports, which is the code under test.

near_ties is run where its clusters spread over several score levels.  On fp32 rows under cosine, and on bf16 rows
under cosine at d = 768 and 3072, the one-ulp moves of an element are lost in the fp32 sum: every member of a cluster
has the SAME canonical score and no threshold can have members on both sides.  bf16 rows under L2 keep 13 to 17 levels
per cluster at d = 768 and 3072 (skinny and 4-wave kernel), and at d = 128 bf16 rows spread under both metrics and fp32
rows under L2: those cases run.  split_worst is also run at d = 16: the split pass's bound is
4.1 * 3 dim u + 3.1 * 2^-16, the family's coherent error is about a quarter of the second term, so only a short row
brings the real error above a tenth of the bound -- the place where a range search whose widening is too small by that
factor loses rows.

At 300 000 rows the threshold is taken among each query's best 4096 rows (the densest rank there): the band is as
populated as at the small sizes and the answers stay a few hundred thousand entries instead of half the corpus.

band_counts() counts, per query, the rows within one bound of the threshold that qualify (n_in) and that do not
(n_out).  The condition every case must meet on the reference alone: n_in >= 1 and n_out >= 1 for at least three
quarters of its queries.
"""
import numpy as np

import certificate_fixtures as F
from support import DT, THREADS, prep_of, form_of

# a range search has no stream form
KERNELS = {name: row for name, row in F.KERNELS.items() if not name.startswith("stream")}
NEAR_TIES_K = 10            # clusters of 3 k + 8 = 38 rows
N_SMALL = 4096              # d = 768 / 3072
N_OFFSET = 20000            # offset_cluster: the widened threshold admits every row; > 8192 so that the lists overflow
N_LARGE, DIM_LARGE = 300_000, 128
DIM_SHORT = 16              # split_worst on the split kernels
LARGE_BEST = 4096           # at N_LARGE: the threshold is a score among the query's best rows
MIN_QUERY_SHARE = 0.75


def _families(dtype, metric):
    if metric == "ip":
        return ["cancel", "range"]
    fam = ["cancel", "range"]
    if dtype == "f32":
        fam.append("split_worst")
    if metric == "l2":
        fam.append("offset_cluster")
    return fam


def cases():
    """(kernel, dim, metric, family, rows).  d = 768 / 3072: every kernel x metric x family.  300 000 x 128: every
    kernel x family once, the metrics dealt in turn (offset_cluster is L2 only; IP on cancel and range).  near_ties:
    bf16 rows under L2 at d = 768 / 3072, under L2 and cosine at d = 128; fp32 rows under L2 at d = 128.  4096 x 16:
    split_worst on the two split kernels."""
    out = []
    for name, (dtype, _, _, _, _, dims) in KERNELS.items():
        for dim in dims:
            for metric in ("cosine", "l2", "ip"):
                for fam in _families(dtype, metric):
                    out.append((name, dim, metric, fam, N_OFFSET if fam == "offset_cluster" else N_SMALL))
            if dtype == "bf16":          # the clusters spread over score levels under L2 only (module docstring)
                out.append((name, dim, "l2", "near_ties", N_SMALL))
    turn = 0
    for name, (dtype, _, _, _, _, _) in KERNELS.items():
        for fam in _families(dtype, "l2"):
            choices = ("l2",) if fam == "offset_cluster" else ("cosine", "l2", "ip") if fam in ("cancel", "range") else ("cosine", "l2")
            out.append((name, DIM_LARGE, choices[turn % len(choices)], fam, N_LARGE))
            turn += 1
        # near_ties: L2 everywhere; cosine on bf16 rows (a one-ulp move of an fp32 element never changes an fp32 dot)
        out += [(name, DIM_LARGE, metric, "near_ties", N_LARGE) for metric in (("l2", "cosine") if dtype == "bf16" else ("l2",))]
    for name, (dtype, _, _, _, split_pass, _) in KERNELS.items():
        if split_pass:
            out += [(name, DIM_SHORT, metric, "split_worst", N_SMALL) for metric in ("cosine", "l2")]
    return out


def case_id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}"


def _norms(p):
    return np.sqrt((p.astype(np.float64) ** 2).sum(axis=1))


def _worse(metric):
    return np.float32(np.inf if metric == "l2" else -np.inf)


def band_counts(sorted_scores, thr, eps, metric):
    """sorted_scores: one query's canonical scores, ascending fp64.  (n_in, n_out): the rows within eps of thr that
    qualify / do not."""
    t = float(thr)
    lo = np.searchsorted(sorted_scores, t - eps, "left")
    hi = np.searchsorted(sorted_scores, t + eps, "right")
    if metric == "l2":      # qualifies: s <= t
        cut = np.searchsorted(sorted_scores, t, "right")
        return int(cut - lo), int(hi - cut)
    cut = np.searchsorted(sorted_scores, t, "left")     # qualifies: s >= t
    return int(hi - cut), int(cut - lo)


def build(O, case):
    """The inputs, thresholds and reference of one case.  Returns a dict: raw, rq (raw fp32), thr, want (lims, ids,
    scores of oracle.scan_range), eps, n_in / n_out (per query), share (of queries with both >= 1)."""
    name, dim, metric, family, n = case
    dtype, _, nq, mode, split_pass, _ = KERNELS[name]
    gen_metric = "cosine" if metric == "ip" else metric
    if family == "near_ties":
        raw, rq, nc = F.near_ties(n, nq, dim, gen_metric, dtype, NEAR_TIES_K, seed=dim + 4)
    else:
        raw, rq = F.make(family, n, nq, dim, gen_metric, dtype, seed=dim)
        nc = 0
    pc = O.prepare(raw, DT[dtype], prep_of(metric), threads=THREADS)
    pq = O.prepare(rq, DT[dtype], prep_of(metric), threads=THREADS)
    eps = float(F.mfma_eps(dim, "l2" if metric == "l2" else "cosine", bool(split_pass), _norms(pq).max(), _norms(pc).max()))
    assert np.isfinite(eps) and eps > 0
    # every row's canonical score, per query best first: the permissive threshold
    lims, _, sc = O.scan_range(pc, pq, _worse(metric), form_of(metric), threads=THREADS)
    assert np.array_equal(lims, np.arange(nq + 1, dtype=np.uint64) * np.uint64(n)), "every score is a number"
    sc = sc.reshape(nq, n)
    m = 3 * NEAR_TIES_K + 8
    thr = np.empty(nq, np.float32)
    asc = []
    for q in range(nq):
        best_first = sc[q]
        s = best_first.astype(np.float64)
        s = s if metric == "l2" else s[::-1]
        asc.append(s)
        kind = q % 3
        if q < nc:
            # a score level of the cluster with members on both sides of the boundary: any level but the worst when the
            # level itself qualifies, any but the best when it does not (one float to the better side)
            levels = np.unique(best_first[:m])
            levels = levels if metric == "l2" else levels[::-1]          # best first
            t = levels[min(len(levels) // 2, len(levels) - 2)] if kind < 2 else levels[max(len(levels) // 2, 1)] if len(levels) > 1 else levels[0]
            t = levels[0] if len(levels) == 1 else t
        else:
            dense = np.searchsorted(s, s + eps, "right") - np.searchsorted(s, s - eps, "left")
            if n == N_LARGE:                               # ranks among the best LARGE_BEST rows only
                if metric == "l2":
                    dense[LARGE_BEST:] = -1
                else:
                    dense[:n - LARGE_BEST] = -1
            top = np.flatnonzero(dense == dense.max())
            t = np.float32(s[int(top[len(top) // 2])])     # (a plateau -- a bound wider than the scores -- : its middle)
        thr[q] = t if kind == 0 else np.nextafter(t, _worse(metric)) if kind == 1 else np.nextafter(t, -_worse(metric))
    counts = np.array([band_counts(asc[q], thr[q], eps, metric) for q in range(nq)])
    want = O.scan_range(pc, pq, thr, form_of(metric), threads=THREADS)
    share = float(np.mean((counts[:, 0] >= 1) & (counts[:, 1] >= 1)))
    return {"raw": raw, "rq": rq, "thr": thr, "want": want, "eps": eps, "n_in": counts[:, 0], "n_out": counts[:, 1],
            "share": share, "nc": nc}


def report(case, c):
    """The line the issue asks for: RANGE_BAND family kernel dim n_in n_out (medians over the queries), then the rest."""
    name, dim, metric, family, n = case
    return (f"RANGE_BAND {family} {name} {dim} {int(np.median(c['n_in']))} {int(np.median(c['n_out']))} "
            f"metric={metric} rows={n} min_in={int(c['n_in'].min())} min_out={int(c['n_out'].min())} share={c['share']:.2f} "
            f"eps={c['eps']:.3e} answer={int(c['want'][0][-1])}")
