"""index_model.ModelIndex with row tags: what a handle must hold, and what vrod_search_tagged must return.

Every row carries one 64-bit tag mask, 0 until set and for rows added later; compact moves the tags with their rows.
A tagged search is the model's one primitive once per distinct predicate: the oracle over the rows that are eligible
(live, allowed) and match it, taken in ascending order.  Labels play no part.
"""
import numpy as np

from index_model import ERR_INVALID_ARG, ID_NONE, ModelError, ModelIndex


def tag_matches(tags, pred):
    """Rows of the uint64 array `tags` that match pred = (any, all, none)."""
    a, b, c = (np.uint64(int(x)) for x in pred)
    zero = np.uint64(0)
    return ((tags & a) != zero if a else np.ones(tags.shape, bool)) & ((tags & b) == b) & ((tags & c) == zero)


def distinct_preds(preds):
    """[nq, 3] uint64 -> the distinct triples as tuples of ints, ordered by the triple."""
    return sorted({tuple(int(x) for x in p) for p in np.asarray(preds, dtype=np.uint64).reshape(-1, 3)})


class TagModelIndex(ModelIndex):
    def __init__(self, dim, dtype, metric, id_offset=0):
        super().__init__(dim, dtype, metric, id_offset)
        self.tags = np.zeros(0, np.uint64)

    def add(self, raw):
        grew = super().add(raw)
        self.tags = np.concatenate([self.tags, np.zeros(self.count - self.tags.size, np.uint64)])
        return grew

    def set_tags(self, first_id, tags):
        tags = np.asarray(tags, dtype=np.uint64).reshape(-1)
        first = int(first_id) - self.offset
        if first < 0 or first > self.count or first + tags.size > self.count:
            raise ModelError(ERR_INVALID_ARG, "set_tags: a range past the rows")
        self.tags = self.tags.copy()
        self.tags[first:first + tags.size] = tags

    def get_tags(self, first_id, n):
        first = int(first_id) - self.offset
        if first < 0 or first > self.count or first + n > self.count:
            raise ModelError(ERR_INVALID_ARG, "get_tags: a range past the rows")
        return self.tags[first:first + n].copy()

    def compact(self, map_len=None):
        keep = ~self.deleted
        new_ids = super().compact(map_len)
        self.tags = self.tags[keep]
        return new_ids

    def matching(self, pred):
        """Ascending local rows query with predicate `pred` sees."""
        return np.flatnonzero(self.eligible() & tag_matches(self.tags, pred))

    def search_tagged(self, rq, k, preds):
        pq = self._queries(rq)
        preds = np.asarray(preds, dtype=np.uint64).reshape(-1, 3)
        ids = np.full((pq.shape[0], k), ID_NONE, np.uint64)
        sc = np.full((pq.shape[0], k), np.nan, np.float32)
        for p in distinct_preds(preds):
            qs = np.flatnonzero((preds == np.array(p, np.uint64)).all(axis=1))
            ids[qs], sc[qs] = self._topk(self.matching(p), np.ascontiguousarray(pq[qs]), k)
        return ids, sc
