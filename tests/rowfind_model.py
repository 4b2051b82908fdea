"""The model of one vrod_index_find_rows / vrod_index_add_unique call, in numpy.

An input equals a stored row when, prepared as add() would store it, its dim elements have the stored row's bits.  The
stored side is what get_rows reads back (a bf16 element widened to fp32 is exact, as in dup_model); the input side is the
CPU oracle's prepare(), which is what add() is tested against.  The model matches by bytes, walks the inputs in call order
with a dict of the call's firsts, and returns the ids, the four exact stats and the inputs an add_unique appends.  It
runs on any fp32 arrays, so it is tested without a GPU (test_rowfind_model.py).
"""
import numpy as np

from support import DT, THREADS, prep_of

ID_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
ROWFIND_NARROW_HASH = 0x80000000
ROWFIND_SMALL_BATCH = 0x40000000
SMALL_ROWS = 96                                        # rowfind_plan.h kRowfindSmallRows
EXACT_STATS = ("rows", "found", "repeats", "appended")


def prepared(O, inputs, dtype, metric):
    """The inputs as add() would store them, read back as fp32."""
    inputs = np.ascontiguousarray(inputs, dtype=np.float32)
    return O.prepare(inputs, DT[dtype], prep_of(metric), threads=THREADS)


def lookup(stored, deleted, prepared_inputs, append, id_offset=0):
    """stored: [count, dim] fp32 as get_rows(0, count) gives them; deleted: local rows; prepared_inputs: [n, dim] fp32.
    -> (out_ids [n] uint64, the four exact stats, the inputs an add_unique appends, in order)."""
    stored = np.ascontiguousarray(stored, dtype=np.float32)
    pin = np.ascontiguousarray(prepared_inputs, dtype=np.float32)
    count, n = stored.shape[0], pin.shape[0]
    live = np.ones(count, bool)
    live[np.asarray(deleted, dtype=np.int64)] = False
    smallest = {}
    for r in np.flatnonzero(live):                                               # ascending: the first seen is the smallest
        smallest.setdefault(stored[r].view(np.uint32).tobytes(), int(r))
    out = np.full(n, ID_NONE, np.uint64)
    firsts, appended = {}, []
    found = repeats = 0
    for i in range(n):
        key = pin[i].view(np.uint32).tobytes()                                   # the bits: -0.0 is not +0.0
        if key in smallest:
            out[i] = np.uint64(smallest[key] + id_offset)
            found += 1
        elif key in firsts:
            out[i] = out[firsts[key]]
            repeats += 1
        else:
            firsts[key] = i
            if append:
                out[i] = np.uint64(count + len(appended) + id_offset)
            appended.append(i)
    stats = {"rows": n, "found": found, "repeats": repeats, "appended": len(appended) if append else 0}
    return out, stats, appended


def of_handle(O, ix, dtype, metric, inputs, deleted=(), append=False):
    """The model of a handle: its rows read back, `deleted` as ids of the handle, its id offset."""
    off = getattr(ix, "_id_offset", 0)
    rows = ix.get_rows(0, ix.count) if ix.count else np.zeros((0, ix.dim), np.float32)   # (get_rows takes rows, not ids)
    dead = np.asarray(deleted, dtype=np.int64) - off
    return lookup(rows, dead, prepared(O, inputs, dtype, metric), append, off)


def exact(stats):
    return {k: int(stats[k]) for k in EXACT_STATS}
