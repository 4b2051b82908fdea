"""The model of one vrod_index_find_near_duplicates call: the CPU oracle's range scan plus a union-find in Python.

The rows are the handle's prepared rows as get_rows reads them back (a bf16 element widened to fp32 is exact), the queries
are those same rows -- nothing is prepared again -- so the scores are the canonical scores between stored rows.  Eligible
rows i != j are joined when j is in i's range answer at the threshold (inclusive, a NaN score never qualifies); the
classes are the connected components, every row is mapped to the smallest row of its class, and a row that is not
eligible to ID_NONE.  It runs on any fp32 array, so it is tested without a GPU (test_near_model.py).
"""
import numpy as np

from support import THREADS, form_of

ID_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
NEAR_SMALL_POOL = 0x80000000
EXACT_STATS = ("rows", "classes", "near_duplicates", "largest_class", "hits")


class SmallestRoot:
    """Union-find whose root is the smallest member: the larger root is linked under the smaller, finds halve paths."""

    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def find_near_duplicates(O, rows, eligible, threshold, form, id_offset=0):
    """rows: [count, dim] fp32 as get_rows(0, count) gives them; eligible: [count] bools; form: the oracle's score form
    (METRIC_COSINE also serves the inner product).  -> (out_first [count] uint64, the five exact stats)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    eligible = np.asarray(eligible, dtype=bool).reshape(-1)
    count = rows.shape[0]
    assert eligible.size == count
    el = np.flatnonzero(eligible)
    out = np.full(count, ID_NONE, np.uint64)
    if el.size == 0:
        return out, dict.fromkeys(EXACT_STATS, 0)
    lims, ids, _ = O.scan_range(rows, rows[el], np.float32(threshold), form, mask=eligible, threads=THREADS)
    a = np.repeat(el, np.diff(lims.astype(np.int64)))                            # the query row of every hit
    b = ids.astype(np.int64)
    other = a != b                                                               # self is dropped and not counted
    hits = int(other.sum())
    # every undirected pair once (the relation is used in both directions whichever side reported it)
    lo, hi = np.minimum(a[other], b[other]), np.maximum(a[other], b[other])
    pairs = np.unique(lo * count + hi)
    uf = SmallestRoot(count)
    for p in pairs.tolist():
        uf.union(p // count, p % count)
    root = np.array([uf.find(int(r)) for r in el], np.int64)
    out[el] = root.astype(np.uint64) + np.uint64(id_offset)
    sizes = np.bincount(root, minlength=count)
    classes = int((root == el).sum())
    stats = {"rows": int(el.size), "classes": classes, "near_duplicates": int(el.size) - classes,
             "largest_class": int(sizes.max()), "hits": hits}
    return out, stats


def of_handle(O, ix, metric, threshold, allow=None, deleted=()):
    """The model of a handle: its rows read back, `deleted` as ids of the handle, `allow` the filter's bools (rows past it
    are not allowed; None: no filter), its id offset."""
    off = getattr(ix, "_id_offset", 0)
    rows = ix.get_rows(0, ix.count) if ix.count else np.zeros((0, ix.dim), np.float32)   # (get_rows takes rows, not ids)
    eligible = np.ones(ix.count, bool)
    if allow is not None:
        eligible[:] = False
        eligible[:len(allow)] = allow
    eligible[np.asarray(deleted, dtype=np.int64) - off] = False
    return find_near_duplicates(O, rows, eligible, threshold, form_of(metric), off)


def exact(stats):
    return {k: int(stats[k]) for k in EXACT_STATS}
