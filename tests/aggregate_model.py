"""rowpred_model.RowPredModelIndex with row aggregation: what vrod_index_aggregate_where must return.

The rows considered are `matching(pred, flags & ALLOWED)`, the rows select_where lists.  Each contributes (key, value,
id) records: one under BY_LABEL (key = its label) and BY_VALUE (key = floor(value / width), numpy's // on int64 is floor
division), one per set tag bit under BY_TAG (key = the bit's index), so a row without tags contributes none.  A group is
the records of one key: their number, the signed min and max of the values, their sum mod 2^64 (added as uint64, read
back as int64: the wrap-around is explicit, not a numpy accident) and the smallest id.  The order is key ascending, or
under ORDER_COUNT count descending and then key ascending.
"""
import numpy as np

from index_model import ERR_INVALID_ARG, ModelError
from rowpred_model import ALLOWED, RowPredModelIndex

BY_LABEL, BY_VALUE, BY_TAG = 0, 1, 2                 # VROD_AGG_BY_*
ORDER_COUNT = 4                                      # VROD_AGG_ORDER_COUNT
MAX_AGG_GROUPS = 1 << 20                             # VROD_MAX_AGG_GROUPS
ERR_CAPACITY = 8
AGG_GROUP_DTYPE = np.dtype([("key", np.int64), ("count", np.uint64), ("min_value", np.int64), ("max_value", np.int64),
                            ("sum_value", np.int64), ("first_id", np.uint64)])


# ---------------------------------------------------------------- aggregate_plan.h restated (tests/test_aggregate_plan.py pins each
# of these against the compiled header; tests/test_gpu_aggregate.py builds its label patterns from them)
LDS_SLOTS, LDS_PROBE, MIN_SLOTS = 512, 8, 1024      # kAggLdsSlots, kAggLdsProbe, kAggMinSlots


def key_hash(keys):
    """keys_plan.h key_hash over an array of keys (any integer dtype, taken mod 2^64) -> uint64."""
    with np.errstate(over="ignore"):
        z = np.asarray(keys).astype(np.int64).view(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def home(keys, slots):
    """agg_home: the global table's home slot, the hash's low bits."""
    return key_hash(keys) & np.uint64(slots - 1)


def lds_home(keys):
    """agg_lds_home: a work-group's LDS table takes the bits from 32 up."""
    return (key_hash(keys) >> np.uint64(32)) & np.uint64(LDS_SLOTS - 1)


def table_slots(count):
    """agg_table_slots: a power of two, at least twice min(count, MAX_AGG_GROUPS) and at least MIN_SLOTS."""
    s = MIN_SLOTS
    while s < 2 * min(int(count), MAX_AGG_GROUPS):
        s *= 2
    return s


def labels_sharing_both_homes(n, slots, like=0):
    """The first n labels, ascending from `like`, whose home slot is `like`'s in the LDS table AND in a global table of
    `slots` slots: about one label in LDS_SLOTS * slots."""
    found, lo, step = [], int(like), 1 << 22
    while len(found) < n:
        k = np.arange(lo, lo + step, dtype=np.int64)
        hit = (lds_home(k) == lds_home([like])[0]) & (home(k, slots) == home([like], slots)[0])
        found += k[hit].tolist()
        lo += step
        assert lo < 1 << 32, "labels are 32 bits"
    return np.array(found[:n], np.uint32)


def records(by, width, labels, values, tags, ids):
    """The (key, value, id) records of some rows, as three arrays."""
    if by == BY_LABEL:
        return labels.astype(np.int64), values, ids
    if by == BY_VALUE:
        return values // np.int64(int(width)), values, ids
    keys, vals, rids = [], [], []
    for b in range(64):
        has = (tags >> np.uint64(b)) & np.uint64(1) != 0
        keys.append(np.full(int(has.sum()), b, np.int64))
        vals.append(values[has])
        rids.append(ids[has])
    return np.concatenate(keys), np.concatenate(vals), np.concatenate(rids)


def fold(keys, values, ids):
    """Records -> the groups by key ascending, an array of AGG_GROUP_DTYPE."""
    order = np.argsort(keys, kind="stable")
    keys, values, ids = keys[order], values[order], ids[order]
    uniq, start = np.unique(keys, return_index=True)
    out = np.zeros(uniq.size, AGG_GROUP_DTYPE)
    if uniq.size:
        out["key"] = uniq
        out["count"] = np.diff(np.append(start, keys.size)).astype(np.uint64)
        out["min_value"] = np.minimum.reduceat(values, start)
        out["max_value"] = np.maximum.reduceat(values, start)
        out["sum_value"] = np.add.reduceat(values.view(np.uint64), start).view(np.int64)   # mod 2^64
        out["first_id"] = np.minimum.reduceat(ids, start)
    return out


def by_count(groups):
    """Groups in the order of ORDER_COUNT: count descending (the complement of an unsigned count ascending), then key."""
    return groups[np.lexsort((groups["key"], ~groups["count"]))]


class AggregateModelIndex(RowPredModelIndex):
    def aggregate_where(self, pred, by, width=None, limit=None, flags=0):
        """-> (the first min(limit, groups) groups in the call's order, groups, rows considered); limit None: every group."""
        if flags & ~(ALLOWED | ORDER_COUNT) or by not in (BY_LABEL, BY_VALUE, BY_TAG):
            raise ModelError(ERR_INVALID_ARG, "unknown flag bits, or an unknown key")
        if by == BY_VALUE and (width is None or int(width) < 1):
            raise ModelError(ERR_INVALID_ARG, "BY_VALUE needs a width of at least 1")
        rows = self.matching(pred, flags & ALLOWED)
        ids = rows.astype(np.uint64) + np.uint64(self.offset)
        groups = fold(*records(by, width, self.labels[rows], self.values[rows].astype(np.int64), self.tags[rows], ids))
        if groups.size > MAX_AGG_GROUPS:
            raise ModelError(ERR_CAPACITY, "more than MAX_AGG_GROUPS groups")
        if flags & ORDER_COUNT:
            groups = by_count(groups)
        return groups[:None if limit is None else int(limit)], int(groups.size), int(rows.size)
