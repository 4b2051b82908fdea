"""The model of one vrod_index_find_duplicates call, in numpy.

Two live rows are duplicates when the dim stored elements of their prepared rows have the same bits.  What the handle
stores is what get_rows reads back (a bf16 element widened to fp32 is exact, so equal fp32 bits there are equal stored
bits), so the model groups the live rows of that array by their bytes -- or by (label, bytes) -- and takes the smallest
id of each group.  It runs on any fp32 array, so it is tested without a GPU (test_dup_abi.py).
"""
import numpy as np

ID_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
DUP_WITHIN_LABEL = 1
DUP_NARROW_HASH = 0x80000000
EXACT_STATS = ("live", "classes", "duplicates", "largest_class")


def find_duplicates(rows, deleted=(), labels=None, within_label=False, id_offset=0):
    """rows: [count, dim] fp32 as get_rows(0, count) gives them; deleted: local rows; labels: [count] uint32 or None (0
    everywhere).  -> (out_first [count] uint64, the four exact stats)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    count = rows.shape[0]
    words = rows.view(np.uint32).reshape(count, rows.shape[1] if rows.ndim == 2 else 0)   # the bits: -0.0 is not +0.0
    live = np.ones(count, bool)
    live[np.asarray(deleted, dtype=np.int64)] = False
    lab = np.zeros(count, np.uint32) if labels is None or not within_label else np.asarray(labels, np.uint32)
    first_of, size = {}, {}
    out = np.full(count, ID_NONE, np.uint64)
    for r in np.flatnonzero(live):                                               # ascending: the first seen is the smallest
        key = (int(lab[r]), words[r].tobytes())
        first_of.setdefault(key, int(r))
        size[key] = size.get(key, 0) + 1
        out[r] = np.uint64(first_of[key] + id_offset)
    n_live = int(live.sum())
    stats = {"live": n_live, "classes": len(first_of), "duplicates": n_live - len(first_of), "largest_class": max(size.values(), default=0)}
    return out, stats


def of_handle(ix, deleted=(), within_label=False, labels=None):
    """The model of a handle: its rows read back, `deleted` as ids of the handle, its id offset."""
    off = getattr(ix, "_id_offset", 0)
    rows = ix.get_rows(0, ix.count) if ix.count else np.zeros((0, ix.dim), np.float32)   # (get_rows takes rows, not ids)
    dead = np.asarray(deleted, dtype=np.int64) - off
    return find_duplicates(rows, dead, labels, within_label, off)


def exact(stats):
    return {k: int(stats[k]) for k in EXACT_STATS}
