"""The model of the candidate-list searches (vrod_search_candidates, vrod_score_candidates): plain numpy and the CPU oracle.

  candidate set   per query, np.unique of its list of ids -- ascending, repeats once -- mapped to local rows and
                  intersected with the eligible rows (support.eligible_rows: live and allowed); an id below the offset,
                  past the count or equal to ID_NONE maps to no row;
  search form     support.oracle_over on that set: what a fresh handle holding only those rows, in ascending id order,
                  returns, ids mapped back;
  score form      the oracle's full-length list of the set (k = its size) scattered back to the caller's positions, NaN
                  wherever the id is not in the set.  A repeated id gets the same score at every position.

Lists are sequences of ids (any uint64 value); `eligible` is ascending local rows; n is the handle's row count.
"""
import numpy as np

from support import ID_NONE, oracle_over


def candidate_rows(ids, n, eligible, id_offset=0):
    """One query's candidate set as ascending local rows (int64)."""
    u = np.unique(np.asarray(ids, dtype=np.uint64))
    u = u[(u != ID_NONE) & (u >= np.uint64(id_offset))]
    rows = (u - np.uint64(id_offset))
    rows = rows[rows < np.uint64(n)].astype(np.int64)
    return np.intersect1d(rows, np.asarray(eligible, np.int64), assume_unique=True)


def search(O, raw, rq, k, dtype, metric, lists, eligible, id_offset=0):
    """-> (ids uint64 [nq, k], scores float32 [nq, k])."""
    nq = len(lists)
    assert rq.shape[0] == nq
    oi = np.full((nq, k), ID_NONE, np.uint64)
    osc = np.full((nq, k), np.nan, np.float32)
    for q in range(nq):
        rows = candidate_rows(lists[q], raw.shape[0], eligible, id_offset)
        oi[q], osc[q] = (a[0] for a in oracle_over(O, raw, np.ascontiguousarray(rq[q][None, :]), k, dtype, metric, rows, id_offset))
    return oi, osc


def score(O, raw, rq, dtype, metric, lists, eligible, id_offset=0):
    """-> scores float32, flat: the lists one after the other, one score per entry."""
    nq = len(lists)
    assert rq.shape[0] == nq
    out = []
    for q in range(nq):
        ids = np.asarray(lists[q], dtype=np.uint64).reshape(-1)
        sc = np.full(ids.size, np.nan, np.float32)
        rows = candidate_rows(ids, raw.shape[0], eligible, id_offset)
        if rows.size:
            fi, fs = (a[0] for a in oracle_over(O, raw, np.ascontiguousarray(rq[q][None, :]), rows.size, dtype, metric, rows, id_offset))
            assert not np.any(fi == ID_NONE)                      # the full-length list names every row of the set once
            order = np.argsort(fi)
            fi, fs = fi[order], fs[order]
            at = np.searchsorted(fi, ids)
            at[at == fi.size] = 0
            hit = fi[at] == ids
            sc[hit] = fs[at[hit]]
        out.append(sc)
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def flat(lists):
    """The lists as the C arguments: (cand_ids uint64, cand_lims uint32 [nq + 1])."""
    lims = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32)
    ids = np.concatenate([np.asarray(l, dtype=np.uint64).reshape(-1) for l in lists]) if lists else np.zeros(0, np.uint64)
    return np.ascontiguousarray(ids, dtype=np.uint64), lims
