"""tag_model.TagModelIndex with a signed 64-bit value per row: what a handle must hold, and what vrod_search_where must
return.

Every row carries one int64 value, 0 until set and for rows added later; compact moves the values with their rows.  A
predicate is (any, all, none, lo, hi): the tag clauses of tag_model.tag_matches and lo <= v <= hi, compared as signed
values with both ends inclusive.  The search is the model's one primitive once per distinct predicate: the oracle over
the rows that are eligible (live, allowed) and match it, taken in ascending order.
"""
import numpy as np

from index_model import ERR_INVALID_ARG, ID_NONE, ModelError
from tag_model import TagModelIndex, tag_matches

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FULL = (I64_MIN, I64_MAX)
WHERE_DTYPE = np.dtype([("any", np.uint64), ("all", np.uint64), ("none", np.uint64), ("lo", np.int64), ("hi", np.int64)])


def as_preds(preds):
    """Tuples (any, all, none, lo, hi) of Python ints, or a structured array -> a [nq] array of WHERE_DTYPE."""
    if isinstance(preds, np.ndarray) and preds.dtype == WHERE_DTYPE:
        return preds.reshape(-1)
    return np.array([tuple(int(x) for x in p) for p in preds], WHERE_DTYPE)


def where_matches(tags, values, pred):
    """Rows of (tags uint64, values int64) that match pred = (any, all, none, lo, hi)."""
    lo, hi = int(pred[3]), int(pred[4])
    return tag_matches(tags, pred[:3]) & (values >= np.int64(lo)) & (values <= np.int64(hi))


def unsatisfiable(pred):
    return int(pred[3]) > int(pred[4]) or (int(pred[1]) & int(pred[2])) != 0


def distinct_preds(preds):
    """-> the distinct predicates as tuples of ints, ordered by (any, all, none, lo, hi) with the ends signed."""
    return sorted({tuple(int(x) for x in p) for p in as_preds(preds).tolist()})


class WhereModelIndex(TagModelIndex):
    def __init__(self, dim, dtype, metric, id_offset=0):
        super().__init__(dim, dtype, metric, id_offset)
        self.values = np.zeros(0, np.int64)

    def add(self, raw):
        grew = super().add(raw)
        self.values = np.concatenate([self.values, np.zeros(self.count - self.values.size, np.int64)])
        return grew

    def _range(self, first_id, n, what):
        first = int(first_id) - self.offset
        if first < 0 or first > self.count or first + n > self.count:
            raise ModelError(ERR_INVALID_ARG, f"{what}: a range past the rows")
        return first

    def set_values(self, first_id, values):
        values = np.asarray(values, dtype=np.int64).reshape(-1)
        first = self._range(first_id, values.size, "set_values")
        self.values = self.values.copy()
        self.values[first:first + values.size] = values

    def get_values(self, first_id, n):
        first = self._range(first_id, n, "get_values")
        return self.values[first:first + n].copy()

    def compact(self, map_len=None):
        keep = ~self.deleted
        new_ids = super().compact(map_len)
        self.values = self.values[keep]
        return new_ids

    def matching(self, pred):
        """Ascending local rows a query with `pred` sees: 3 entries = a tag predicate, 5 = with the interval."""
        if len(pred) == 3:
            return super().matching(pred)
        return np.flatnonzero(self.eligible() & where_matches(self.tags, self.values, pred))

    def search_where(self, rq, k, preds):
        pq = self._queries(rq)
        preds = as_preds(preds)
        ids = np.full((pq.shape[0], k), ID_NONE, np.uint64)
        sc = np.full((pq.shape[0], k), np.nan, np.float32)
        for p in distinct_preds(preds):
            qs = np.flatnonzero(preds == np.array(p, WHERE_DTYPE))
            ids[qs], sc[qs] = self._topk(self.matching(p), np.ascontiguousarray(pq[qs]), k)
        return ids, sc
