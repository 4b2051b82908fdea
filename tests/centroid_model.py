"""aggregate_model.AggregateModelIndex with group centroids: what vrod_index_centroids_where must return, bit for bit.

The rows considered are `matching(pred, flags & ALLOWED)`; their keys are aggregate_model's (BY_LABEL, BY_VALUE), the group
records aggregate_where's key, count and first_id.  The vectors restate the definition of DESIGN.md "Group centroids" in
numpy and Python ints.  x: an element of `prepared()`, what get_rows reads back.  n: the handle's rows, deleted ones
included; R = n.bit_length(), the smallest integer with n < 2^R.
  1. E = 1 under cosine; otherwise m = max(bits(x) & 0x7fffffff) over the considered rows, m >= 0x7f800000 is
     ERR_INVALID_ARG, else E = max(m >> 23, 1) - 126.
  2. s = 62 - R - E.
  3. q = rint(float64(x) * 2^s) as int64: the product is exact, numpy's rint rounds ties to even.
  4. S = the sum of q over the group's rows: an int64 sum that cannot wrap (test_centroid_model.py checks it against
     Python ints at the edge), so numpy's reduction order decides nothing.
  5. sums: float32(float64(S) * 2^-s); means: float32((float64(S) / float64(count)) * 2^-s).  astype rounds to nearest
     even, int64 -> float64 included.
"""
import numpy as np

from aggregate_model import BY_LABEL, BY_VALUE, AggregateModelIndex, records
from index_model import ERR_INVALID_ARG, ModelError
from rowpred_model import ALLOWED

CENTROID_SUM = 8                                     # VROD_CENTROID_SUM
MAX_CENTROID_GROUPS = 1 << 16                        # VROD_MAX_CENTROID_GROUPS
ERR_CAPACITY = 8
NON_FINITE = 0x7F800000
CENTROID_GROUP_DTYPE = np.dtype([("key", np.int64), ("count", np.uint64), ("first_id", np.uint64)])


def row_bits(n):
    """R: the smallest integer with n < 2^R."""
    return int(n).bit_length()


def abs_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def exponent(m):
    """E from m = max(bits(x) & 0x7fffffff) < NON_FINITE: every |x| < 2^E."""
    return max(int(m) >> 23, 1) - 126


def scale(n, E):
    return 62 - row_bits(n) - E


def pow2(k):
    return float(np.ldexp(np.float64(1.0), int(k)))


def quantise(x, s):
    """q = llrint(double(x) * 2^s), an int64 array of x's shape."""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * pow2(s)).astype(np.int64)


def sum_value(S, s):
    with np.errstate(over="ignore"):
        return (np.asarray(S, np.int64).astype(np.float64) * pow2(-s)).astype(np.float32)


def mean_value(S, count, s):
    with np.errstate(over="ignore"):
        return ((np.asarray(S, np.int64).astype(np.float64) / np.asarray(count, np.uint64).astype(np.float64)) * pow2(-s)).astype(np.float32)


def centroids(x, keys, n, cosine, sums):
    """Considered rows x [m, dim] with their keys, on a handle of n rows -> (ascending keys, counts, vectors float32)."""
    dim = x.shape[1]
    if x.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64), np.zeros((0, dim), np.float32)
    if cosine:
        E = 1
    else:
        m = int(abs_bits(x).max())
        if m >= NON_FINITE:
            raise ModelError(ERR_INVALID_ARG, "a considered row holds an infinity or a NaN")
        E = exponent(m)
    s = scale(n, E)
    order = np.argsort(keys, kind="stable")
    uniq, start = np.unique(keys[order], return_index=True)
    S = np.add.reduceat(quantise(x[order], s), start, axis=0)
    counts = np.diff(np.append(start, keys.size)).astype(np.uint64)
    return uniq, counts, sum_value(S, s) if sums else mean_value(S, counts[:, None], s)


class CentroidModelIndex(AggregateModelIndex):
    def centroids_where(self, pred, by, width=None, capacity=None, flags=0):
        """-> (groups of CENTROID_GROUP_DTYPE by key ascending, vectors [groups, dim] float32, rows considered)."""
        if flags & ~(ALLOWED | CENTROID_SUM) or by not in (BY_LABEL, BY_VALUE):
            raise ModelError(ERR_INVALID_ARG, "unknown flag bits, or a key that is not BY_LABEL or BY_VALUE")
        if by == BY_VALUE and (width is None or int(width) < 1):
            raise ModelError(ERR_INVALID_ARG, "BY_VALUE needs a width of at least 1")
        if capacity is not None and not 1 <= int(capacity) <= MAX_CENTROID_GROUPS:
            raise ModelError(ERR_INVALID_ARG, "capacity must be in 1..MAX_CENTROID_GROUPS")
        agg, n_groups, n_rows = self.aggregate_where(pred, by, width, None, flags & ALLOWED)
        if n_groups > (MAX_CENTROID_GROUPS if capacity is None else int(capacity)):
            raise ModelError(ERR_CAPACITY, "more groups than the capacity")
        rows = self.matching(pred, flags & ALLOWED)
        keys = records(by, width, self.labels[rows], self.values[rows].astype(np.int64), self.tags[rows], rows)[0]
        uniq, counts, vectors = centroids(self.prepared()[rows], keys, self.count, self.metric == "cosine", bool(flags & CENTROID_SUM))
        groups = np.zeros(n_groups, CENTROID_GROUP_DTYPE)
        for name in CENTROID_GROUP_DTYPE.names:
            groups[name] = agg[name]
        assert np.array_equal(uniq, groups["key"]) and np.array_equal(counts, groups["count"])
        return groups, vectors, n_rows
