"""where_model.WhereModelIndex with the row-predicate operations: what vrod_index_count_where, _select_where,
_delete_where, _set_filter_where and _set_tags_where must do to a handle.

A predicate is (any, all, none, lo, hi, label, has_label): the clauses of where_model.where_matches and, when has_label
is 1, label == the row's label.  The scope of an operation is the live rows (flags 0), or the live rows the filter allows
(flags 1 = ALLOWED); set_filter_where alone looks at every row below the count, deleted or not.  `matching` is the one
primitive; the five mutations are expressed through the model's own delete / set_filter / set_tags, so whatever the
library does must be indistinguishable from the id-based calls.
"""
import numpy as np

from index_model import ERR_INVALID_ARG, ModelError
from where_model import I64_MAX, I64_MIN, WhereModelIndex, unsatisfiable, where_matches

ALLOWED = 1                                          # VROD_ROWPRED_ALLOWED
MATCH_ALL = (0, 0, 0, I64_MIN, I64_MAX, 0, 0)
ROWPRED_DTYPE = np.dtype([("any", np.uint64), ("all", np.uint64), ("none", np.uint64), ("lo", np.int64), ("hi", np.int64),
                          ("label", np.uint32), ("has_label", np.uint32)])


def row_pred_matches(tags, values, labels, pred):
    """Rows of (tags uint64, values int64, labels uint32) that match pred."""
    m = where_matches(tags, values, pred[:5])
    return m & (labels == np.uint32(int(pred[5]))) if int(pred[6]) else m


def _check(pred, flags):
    if int(pred[6]) not in (0, 1):
        raise ModelError(ERR_INVALID_ARG, "has_label is not 0 or 1")
    if flags & ~ALLOWED:
        raise ModelError(ERR_INVALID_ARG, "unknown flag bits")


class RowPredModelIndex(WhereModelIndex):
    def hits(self, pred):
        """bool [count]: the rows that match, whatever their state."""
        if unsatisfiable(pred[:5]):
            return np.zeros(self.count, bool)
        return row_pred_matches(self.tags, self.values, self.labels, pred)

    def scope(self, flags):
        return self.eligible() if flags & ALLOWED else ~self.deleted

    def matching(self, pred, flags=None):
        """Ascending local rows: of a 3- or 5-entry predicate what a query sees (the parent's), of a 7-entry one the rows
        in the scope of `flags` that match."""
        if len(pred) != 7:
            return super().matching(pred)
        _check(pred, flags or 0)
        return np.flatnonzero(self.scope(flags or 0) & self.hits(pred))

    def count_where(self, preds, flags=0):
        return np.array([self.matching(p, flags).size for p in preds], np.uint64)

    def select_where(self, pred, flags=0):
        return self.matching(pred, flags).astype(np.uint64) + np.uint64(self.offset)

    def delete_where(self, pred, flags=0):
        ids = self.select_where(pred, flags)
        self.delete(ids)
        return int(ids.size)

    def filter_bits(self, pred, flags=0):
        """The allow list set_filter_where sets: a row's entry says whether it matches, deleted or not; under ALLOWED also
        whether the filter that is set allows it."""
        _check(pred, flags)
        bits = self.hits(pred)
        if flags & ALLOWED and self.allow is not None:
            bits = bits & self.allow
        return bits

    def set_filter_where(self, pred, flags=0):
        self.set_filter(self.filter_bits(pred, flags))

    def set_tags_where(self, pred, set_bits, clear_bits, flags=0):
        if int(set_bits) & int(clear_bits):
            raise ModelError(ERR_INVALID_ARG, "set_bits and clear_bits share bits")
        rows = self.matching(pred, flags)
        new = self.tags.copy()
        new[rows] = (new[rows] & ~np.uint64(int(clear_bits))) | np.uint64(int(set_bits))
        changed = int((new != self.tags).sum())
        if changed:
            self.set_tags(self.offset, new)
        return changed
