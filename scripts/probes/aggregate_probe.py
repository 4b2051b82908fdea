"""What row aggregation costs against its two yardsticks: 10M x 8 bf16 cosine, rows from add_synthetic (the vectors are
irrelevant), the geometry of order_probe.py.  A row's value is uniform in [0, 3650 days) of seconds; its tags hold a
random mask of ten data bits (0 .. 9, each with probability one half) and one of ten selector bits (16 + t % 10: any =
1 << 16 selects ~10 % of the rows); its label is uniform in 0 .. cardinality - 1 for each cardinality in turn.

Cases: BY_LABEL at cardinality 1, 10, 1000 and 1,000,000, BY_TAG (the ten data bits and the selector bits the predicate
leaves), BY_VALUE with width one day (about 3650 buckets); each without a predicate and with the ~10 % tag predicate.

Yardsticks, measured in the same process on the same handle:
  - select_where of the same predicate: the column-read floor of this geometry (a hit pass, a prefix, a scatter);
  - the host route a caller had before the call: select_where for the rows, get_labels / get_values / get_tags of the
    columns the answer needs, then a stable argsort and numpy reduceat per aggregate (numpy.unique's own method).  Its
    result is compared with the call's, every field, before a time is reported.

Median and minimum wall time of --calls calls after --warmup, one JSON line per case.

    python scripts/probes/aggregate_probe.py [--rows 10000000] [--calls 20] [--warmup 3] > aggregate_probe_10Mx8.jsonl
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
TAGGED = (1 << 16, 0, 0, I64_MIN, I64_MAX, 0, 0)
DAY = 86400


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


def fold(keys, values, ids):
    """(key, value, id) records -> groups by key ascending, as numpy.unique does it: a stable sort, then reduceat."""
    order = np.argsort(keys, kind="stable")
    keys, values, ids = keys[order], values[order], ids[order]
    uniq, start = np.unique(keys, return_index=True)
    out = np.zeros(uniq.size, va.AGG_GROUP_DTYPE)
    if uniq.size:
        out["key"], out["count"] = uniq, np.diff(np.append(start, keys.size))
        out["min_value"], out["max_value"] = np.minimum.reduceat(values, start), np.maximum.reduceat(values, start)
        out["sum_value"] = np.add.reduceat(values.view(np.uint64), start).view(np.int64)
        out["first_id"] = np.minimum.reduceat(ids, start)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2, help="calls of the host route (seconds each at 10M rows)")
    a = ap.parse_args()

    def emit(rec):
        print(json.dumps(rec), flush=True)
    emit({"probe": "aggregate", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)})
    n = a.rows
    rng = np.random.default_rng(17)
    ix = va.Index(8, "bf16", "cosine")
    ix.reserve(n)
    ix.add_synthetic(1, 0, n)
    ix.set_tags(0, rng.integers(0, 1 << 10, n).astype(np.uint64) | (np.uint64(1 << 16) << rng.integers(0, 10, n).astype(np.uint64)))
    ix.set_values(0, rng.integers(0, 3650 * DAY, n).astype(np.int64))

    def host_route(pred, by, width):
        ids = ix.select_where(pred)
        rows = ids.astype(np.int64)
        vals = ix.get_values(0, n)[rows]
        if by == va.AGG_BY_LABEL:
            return fold(ix.get_labels(0, n)[rows].astype(np.int64), vals, ids)
        if by == va.AGG_BY_VALUE:
            return fold(vals // width, vals, ids)
        tags = ix.get_tags(0, n)[rows]
        has = [(tags >> np.uint64(b)) & np.uint64(1) != 0 for b in range(64)]
        return fold(np.concatenate([np.full(int(h.sum()), b, np.int64) for b, h in enumerate(has)]), np.concatenate([vals[h] for h in has]),
                    np.concatenate([ids[h] for h in has]))

    floor = {}
    for what, pred in (("all", MATCH_ALL), ("tag_10pct", TAGGED)):
        floor[what] = timed(lambda: ix.select_where(pred, capacity=n), a.warmup, a.calls)
        emit({"what": f"select_where_{what}", "rows": int(floor[what][2].size), "ms_median": round(floor[what][0], 4), "ms_min": round(floor[what][1], 4)})

    def case(name, by, width):
        for what, pred in (("all", MATCH_ALL), ("tag_10pct", TAGGED)):
            new = timed(lambda: ix.aggregate_where(pred, by, width=width), a.warmup, a.calls)
            count_only = timed(lambda: ix.aggregate_where(pred, by, width=width, limit=0), a.warmup, a.calls)
            top = timed(lambda: ix.aggregate_where(pred, by, width=width, limit=10, by_count=True), a.warmup, a.calls)
            old = timed(lambda: host_route(pred, by, width), 0, a.host_calls)
            groups, n_groups, n_rows = new[2]
            assert groups.tobytes() == old[2].tobytes() and n_groups == old[2].size and n_rows == floor[what][2].size   # the same answer
            emit({"what": f"{name}_{what}", "groups": n_groups, "rows": n_rows, "new_ms_median": round(new[0], 4), "new_ms_min": round(new[1], 4),
                  "count_only_ms_median": round(count_only[0], 4), "top10_by_count_ms_median": round(top[0], 4),
                  "select_where_ms_median": round(floor[what][0], 4), "host_route_ms_median": round(old[0], 2), "host_route_ms_min": round(old[1], 2),
                  "ratio_new_over_select_where": round(new[0] / floor[what][0], 2), "ratio_host_over_new": round(old[0] / new[0], 1)})

    for card in (1, 10, 1000, 1_000_000):
        ix.set_labels(0, rng.integers(0, card, n).astype(np.uint32))
        case(f"by_label_card{card}", va.AGG_BY_LABEL, None)
    case("by_tag", va.AGG_BY_TAG, None)
    case("by_value_day", va.AGG_BY_VALUE, DAY)
    ix.close()


if __name__ == "__main__":
    main()
