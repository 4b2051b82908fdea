"""What ordered selection costs against the route the ABI offered before it: 10M x 8 bf16 cosine, rows from add_synthetic
(the vectors are irrelevant).  A row's value is a uniform random int64, its tags hold a 10-way value (tag bit t % 10 set:
any = 1 selects ~10 % of the rows), its label is uniform in 0 .. 999.

select_ordered is timed with limit in {10, 100, 1000, 65536}, ascending and descending, without a predicate and with
"tag bit 0" (~10 %), then again on a handle whose values column was never set: one tie class, the select's 8-round worst
case.  The comparison is what a caller does without the call for the same answer: select_where for the matching ids,
get_values over the whole column, numpy.lexsort on the host -- timed in the same process against the same handle, and
the two results are compared before a time is reported.

Median and minimum wall time of --calls calls after --warmup, one JSON line per measurement, with the bytes the filter
pass must read (8 B of value per row, + 8 B of tags per row under a tag predicate) and the GB/s that implies.

    python scripts/probes/order_probe.py [--rows 10000000] [--calls 20] [--warmup 3] > order_probe_10Mx8.jsonl
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
MATCH_ALL = (0, 0, 0, I64_MIN, I64_MAX, 0, 0)
TAGGED = (1, 0, 0, I64_MIN, I64_MAX, 0, 0)


def timed(fn, warmup, calls):
    out, last = [], None
    for b in range(warmup + calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        if b >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3, help="calls of the host route (seconds each at 10M rows)")
    a = ap.parse_args()

    def emit(rec):
        print(json.dumps(rec), flush=True)
    emit({"probe": "order", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)})
    n = a.rows
    rng = np.random.default_rng(17)
    ix = va.Index(8, "bf16", "cosine")
    ix.reserve(n)
    ix.add_synthetic(1, 0, n)
    ix.set_tags(0, np.uint64(1) << rng.integers(0, 10, n).astype(np.uint64))
    ix.set_labels(0, rng.integers(0, 1000, n).astype(np.uint32))

    def host_route(pred, limit, desc):
        ids = ix.select_where(pred)
        vals = ix.get_values(0, n)[ids.astype(np.int64)]
        order = np.lexsort((ids, ~vals if desc else vals))[:limit]
        return ids[order], vals[order]

    def cases(column):
        for what, pred, tag_bytes in (("all", MATCH_ALL, 0), ("tag_10pct", TAGGED, 8)):
            host = {}
            for desc in (False, True):
                old = timed(lambda: host_route(pred, 65536, desc), 1, a.host_calls)
                host[desc] = old
            for limit in (10, 100, 1000, 65536):
                for desc in (False, True):
                    new = timed(lambda: ix.select_ordered(pred, limit, desc=desc), a.warmup, a.calls)
                    dev = timed(lambda: ix.select_ordered_device(pred, limit, desc=desc)[:2], a.warmup, a.calls)
                    old = host[desc]
                    assert np.array_equal(new[2][0], old[2][0][:limit]) and np.array_equal(new[2][1], old[2][1][:limit])
                    read = n * (8 + tag_bytes)
                    emit({"what": f"select_ordered_{column}_{what}_limit{limit}_{'desc' if desc else 'asc'}", "total": int(new[2][2]),
                          "new_ms_median": round(new[0], 4), "new_ms_min": round(new[1], 4), "device_form_ms_median": round(dev[0], 4),
                          "host_route_ms_median": round(old[0], 2), "host_route_ms_min": round(old[1], 2), "filter_bytes_read": read,
                          "implied_GBps": round(read / (new[0] * 1e-3) / 1e9, 1), "ratio_host_over_new": round(old[0] / new[0], 1)})

    cases("never_set")                                                           # one tie class: all 8 rounds, pivot = 0
    ix.set_values(0, rng.integers(I64_MIN, I64_MAX, n, endpoint=True))
    cases("random")
    # a cursor in the middle of the listing: the same passes over half the rows
    mid = (0, 0)
    new = timed(lambda: ix.select_ordered(MATCH_ALL, 1000, after=mid), a.warmup, a.calls)
    emit({"what": "select_ordered_random_all_limit1000_asc_after_(0,0)", "total": int(new[2][2]), "new_ms_median": round(new[0], 4),
          "new_ms_min": round(new[1], 4)})
    ix.close()


if __name__ == "__main__":
    main()
