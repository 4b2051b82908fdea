"""What the row-predicate operations cost against the route the ABI offered before them: 10M x 768 bf16 cosine, rows from
add_synthetic.  A row's tags hold a 10-bit value in bits 0 .. 9, its value is uniform in 0 .. 999999 (so the interval
[0, 999] holds ~0.1 % of the rows, [0, 99999] ~10 %), its label is uniform in 0 .. 99 (~1 % of the rows each).

Every operation is timed twice in one process: through the new entry point, and through the host route that gives the
same result -- get_tags + get_values + get_labels (the three columns to the host), a numpy predicate, then delete(ids) /
set_filter(bits) where the operation changes the handle.  The two results are compared before a time is reported.

  count_where       1 predicate; a full table of 1024 distinct predicates (the host route is timed on 8 of them and
                    scaled: a numpy pass per predicate);
  select_where      ~0.1 %, ~10 % and 100 % of the rows;
  delete_where      one label (~1 %) per call, a fresh label every call: the new route's calls, then the host route's;
  set_filter_where  one label (~1 %).

Median and minimum wall time per call, one JSON line per measurement, with the bytes the operation must read (20 B per
row: 8 tags + 8 value + 4 label, plus one bit per row once rows are deleted) and the GB/s that implies.

    python scripts/probes/rowpred_probe.py [--rows 10000000] [--batches 5] [--warmup 2] > rowpred_probe_10Mx768.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import vrod_amd as va  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def timed(fn, warmup, batches):
    out, last = [], None
    for b in range(warmup + batches):
        torch.cuda.synchronize()
        t = time.perf_counter()
        last = fn(b)
        torch.cuda.synchronize()
        if b >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    def emit(rec):
        print(json.dumps(rec), flush=True)
    emit({"probe": "rowpred", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)})
    n = a.rows
    rng = np.random.default_rng(13)
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(n)
    ix.add_synthetic(1, 0, n)
    ix.set_tags(0, rng.integers(0, 1024, n).astype(np.uint64))
    ix.set_values(0, rng.integers(0, 1_000_000, n))
    ix.set_labels(0, rng.integers(0, 100, n).astype(np.uint32))

    def columns():
        return ix.get_tags(0, n), ix.get_values(0, n), ix.get_labels(0, n)

    def host_hits(cols, p):
        t, v, lab = cols
        any_, all_, none, lo, hi, label, has = (int(x) for x in p)
        m = (v >= lo) & (v <= hi)
        if any_:
            m &= (t & np.uint64(any_)) != 0
        if all_:
            m &= (t & np.uint64(all_)) == np.uint64(all_)
        if none:
            m &= (t & np.uint64(none)) == 0
        if has:
            m &= lab == np.uint32(label)
        return m

    def report(what, new, old, rows_read, extra=None):
        (nm, nmin, _), (om, omin, _) = new, old
        rec = {"what": what, "new_ms_median": round(nm, 4), "new_ms_min": round(nmin, 4), "host_route_ms_median": round(om, 3),
               "host_route_ms_min": round(omin, 3), "bytes_read": rows_read, "implied_GBps": round(rows_read / (nm * 1e-3) / 1e9, 1),
               "ratio_host_over_new": round(om / nm, 1)}
        rec.update(extra or {})
        emit(rec)

    col_bytes = n * 20

    # ---- count_where
    one = (0, 0, 0, 0, 99_999, 7, 1)
    new = timed(lambda b: ix.count_where([one]), a.warmup, a.batches)
    old = timed(lambda b: int(host_hits(columns(), one).sum()), a.warmup, a.batches)
    assert int(new[2][0]) == old[2]
    report("count_where_1_predicate", new, old, col_bytes, {"count": old[2]})
    table = np.array([(0, t, ~t & 0x3FF, 0, 499_999, 0, 0) for t in range(1024)], va.ROWPRED_DTYPE)
    new = timed(lambda b: ix.count_where(table), a.warmup, a.batches)

    def host_table(b):
        cols = columns()
        return [int(host_hits(cols, table[i].tolist()).sum()) for i in range(8)]
    old8 = timed(host_table, 1, 3)
    assert new[2][:8].tolist() == old8[2]
    cols_ms = timed(lambda b: columns(), 1, 3)[0]
    scaled = cols_ms + (old8[0] - cols_ms) * 128
    report("count_where_full_table_1024", new, (scaled, scaled, None), col_bytes,
           {"host_route_note": "8 predicates timed (%.1f ms with the columns' copy of %.1f ms), the numpy part scaled x128" % (old8[0], cols_ms)})

    # ---- select_where
    for what, p in (("select_where_0p1pct", (0, 0, 0, 0, 999, 0, 0)), ("select_where_10pct", (0, 0, 0, 0, 99_999, 0, 0)),
                    ("select_where_100pct", (0, 0, 0, I64_MIN, I64_MAX, 0, 0))):
        m = int(ix.count_where([p])[0])
        new = timed(lambda b: ix.select_where(p, capacity=m), a.warmup, a.batches)
        old = timed(lambda b: np.flatnonzero(host_hits(columns(), p)).astype(np.uint64), a.warmup, a.batches)
        assert np.array_equal(new[2], old[2])
        dev = timed(lambda b: ix.select_where_device(p, m), a.warmup, a.batches)
        assert dev[2][0] == 0 and dev[2][1] == m
        report(what, new, old, col_bytes, {"selected": m, "ids_bytes_written": m * 8, "device_form_ms_median": round(dev[0], 4),
                                          "device_form_ms_min": round(dev[1], 4)})

    # ---- set_filter_where: one label
    p = (0, 0, 0, I64_MIN, I64_MAX, 42, 1)
    new = timed(lambda b: (ix.set_filter_where(p), ix.filter_count())[1], a.warmup, a.batches)
    old = timed(lambda b: (ix.set_filter(host_hits(columns(), p)), ix.filter_count())[1], a.warmup, a.batches)
    assert new[2] == old[2]
    report("set_filter_where_1pct", new, old, col_bytes, {"allowed": old[2]})
    ix.set_filter(None)

    # ---- delete_where: a fresh label per call
    labels = iter(range(100))

    def new_delete(b):
        return ix.delete_where((0, 0, 0, I64_MIN, I64_MAX, next(labels), 1))

    def old_delete(b):
        ids = np.flatnonzero(host_hits(columns(), (0, 0, 0, I64_MIN, I64_MAX, next(labels), 1))).astype(np.uint64)   # (a fresh label: all of its rows are live)
        ix.delete(ids)
        return int(ids.size)
    new = timed(new_delete, a.warmup, a.batches)
    old = timed(old_delete, a.warmup, a.batches)
    assert ix.live_count() == n - int(np.isin(ix.get_labels(0, n), np.arange(2 * (a.warmup + a.batches))).sum())
    report("delete_where_1pct", new, old, col_bytes + n // 8, {"deleted_last_call": int(new[2]), "host_route_deleted_last_call": old[2]})
    ix.close()


if __name__ == "__main__":
    main()
