"""The model of a multi-vector search (vrod_search_multivec): ModelIndex plus MaxSim over the row labels.

Everything comes from the oracle's existing functions: M(t, L) is `_topk(rows of L, prepared vectors, 1)`, S(q, L) is built
by explicit np.float32 adds in vector order from +0.0, and the ranking is a lexsort (NaN last, then the score, then the
label).  `routes` mirrors the host decisions of vrod_amd/csrc/multivec_plan.h in Python (tests/test_multivec_plan.py
checks the mirror against the compiled header): which queries the candidate route certifies, from the oracle's own top-k1
lists.
"""
import numpy as np

from index_model import ID_NONE, METRIC_L2, ModelIndex
from support import MAX_K, first_k    # (both are part of this mirror: test_multivec_plan.py checks them against the header)

MAX_QUERY_VECTORS = 256
BATCH_VECTORS = 2048
DENSE_SHARE = 4


# ---- multivec_plan.h, mirrored


def cut(lims, q0, max_vectors=BATCH_VECTORS):
    nq = len(lims) - 1
    q1 = q0 + 1
    while q1 < nq and lims[q1 + 1] - lims[q0] <= max_vectors:
        q1 += 1
    return q1


def lists_complete(any_short, k1, eligible):
    return bool(any_short) or k1 >= eligible


def certified(complete, n_candidates, k, kth, U, higher):
    if complete:
        return True
    if n_candidates < k:
        return False
    return bool(kth > U) if higher else bool(kth < U)


def too_broad(candidate_rows, stored_rows):
    return candidate_rows * DENSE_SHARE > stored_rows


def fl_sum(values):
    """+0.0f + v[0] + v[1] + ... in fp32, one rounding per add."""
    s = np.float32(0.0)
    with np.errstate(all="ignore"):
        for v in values:
            s = np.float32(s + np.float32(v))
    return s


class MultivecModel(ModelIndex):
    def _tables(self, pv):
        """-> (present labels ascending [D], M [nv, D]): the oracle's top-1 of every prepared vector over each label's
        eligible rows."""
        elig = self.eligible()
        present = np.unique(self.labels[elig])
        M = np.empty((pv.shape[0], present.size), np.float32)
        for j, L in enumerate(present):
            M[:, j] = self._topk(np.flatnonzero(elig & (self.labels == L)), pv, 1)[1][:, 0]
        return present.astype(np.uint32), M

    def scores_multivec(self, raw_vectors, lims):
        """-> (present labels [D], S [nq, D])."""
        lims = np.asarray(lims, dtype=np.int64)
        present, M = self._tables(self._queries(raw_vectors))
        S = np.zeros((lims.size - 1, present.size), np.float32)
        with np.errstate(all="ignore"):
            for q in range(lims.size - 1):
                for t in range(lims[q], lims[q + 1]):        # explicit fp32 adds, left to right, from +0.0
                    S[q] = (S[q] + M[t]).astype(np.float32)
        return present, S

    def rank(self, present, S, k):
        nq = S.shape[0]
        ol = np.zeros((nq, k), np.uint32)
        osc = np.full((nq, k), np.nan, np.float32)
        m = min(k, present.size)
        for q in range(nq):
            nan = np.isnan(S[q])
            val = np.where(nan, np.float32(0), S[q] if self.form == METRIC_L2 else -S[q])
            o = np.lexsort((present, val, nan))[:m]          # NaN last, then the score, then the label
            ol[q, :m], osc[q, :m] = present[o], S[q][o]
        return ol, osc, np.full(nq, m, np.uint32)

    def search_multivec(self, raw_vectors, lims, k):
        """-> (labels uint32 [nq, k], scores float32 [nq, k], found uint32 [nq])."""
        present, S = self.scores_multivec(raw_vectors, lims)
        return self.rank(present, S, k)

    def routes(self, raw_vectors, lims, k, present=None, S=None):
        """Per query: True = the candidate route certifies it (multivec_plan.h), False = it goes to the dense route.
        -> (bool [nq], k1)."""
        lims = np.asarray(lims, dtype=np.int64)
        if present is None:
            present, S = self.scores_multivec(raw_vectors, lims)
        elig = self.eligible()
        n_elig = int(elig.sum())
        k1 = first_k(k, n_elig)
        ids, sc = self._topk(np.flatnonzero(elig), self._queries(raw_vectors), k1)
        higher = self.form != METRIC_L2
        rows_of = {int(L): int((elig & (self.labels == L)).sum()) for L in present}
        col = {int(L): j for j, L in enumerate(present)}
        out = np.zeros(lims.size - 1, bool)
        for q in range(lims.size - 1):
            i, s = ids[lims[q]:lims[q + 1]], sc[lims[q]:lims[q + 1]]
            real = i != ID_NONE
            if not np.isfinite(s[real]).all():
                continue
            cands = np.unique(self.labels[(i[real] - np.uint64(self.offset)).astype(np.int64)])
            if too_broad(sum(rows_of[int(L)] for L in cands), self.count):
                continue
            cols = [col[int(L)] for L in cands]
            ol, osc, found = self.rank(cands.astype(np.uint32), S[q:q + 1, cols], k)
            kth = osc[0, k - 1] if found[0] >= k else np.float32(np.nan)
            U = fl_sum(s[:, k1 - 1])
            out[q] = certified(lists_complete(not real.all(), k1, n_elig), cands.size, k, kth, U, higher)
        return out, k1
