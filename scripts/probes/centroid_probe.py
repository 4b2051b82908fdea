"""What group centroids cost against their two yardsticks: rows x 768 bf16 cosine from add_synthetic, three label layouts.

  documents   contiguous runs of about 12 rows, a label per run.  A call holds at most MAX_CENTROID_GROUPS groups, so the
              predicate (a value interval; a row's value is its number) keeps the first 60000 documents;
  random1000  1000 labels at random over every row: every work-group feeds every group;
  one_label   one group of every row.

Yardsticks, measured in the same process on the same handle:
  - the host route a caller had before the call: get_rows of the considered range, get_labels, a stable argsort and
    numpy.add.reduceat in fp64.  Its mean is compared with the call's within the bound of the definition,
    |out - mean64| <= 2^-s + ulp32(mean64), before a time is reported.  It needs 3 KB of host memory a row and seconds
    a call, so it is timed --host-calls times; --no-host-route leaves it out (10M rows are 30 GB);
  - the bytes of the considered rows per second, against the stream scan's rate (README.md).
Beside them aggregate_where of the same arguments, count-only and with every group returned: what the groups alone cost,
the host's ordering of them included.

The call is the device form (the vectors stay in a torch tensor).  Median and minimum wall time of --calls calls after
--warmup, around a device synchronise, one JSON line per case.

    python scripts/probes/centroid_probe.py [--rows 1000000] [--calls 20] [--warmup 3] [--no-host-route] > centroid_probe_1Mx768.jsonl
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
DIM, DOCS = 768, 60000


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
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2, help="calls of the host route (seconds each)")
    ap.add_argument("--no-host-route", dest="host_route", action="store_false",
                    help="skip get_rows + get_labels + numpy, and with it the comparison (3 KB of host memory a row)")
    a = ap.parse_args()

    def emit(rec):
        print(json.dumps(rec), flush=True)
    emit({"probe": "centroid", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)})
    n = a.rows
    rng = np.random.default_rng(23)
    ix = va.Index(DIM, "bf16", "cosine")
    ix.reserve(n)
    ix.add_synthetic(1, 0, n)
    ix.set_values(0, np.arange(n, dtype=np.int64))
    out = torch.empty((va.MAX_CENTROID_GROUPS, DIM), dtype=torch.float32, device="cuda")
    quantum = 2.0 ** -(62 - int(n).bit_length() - 1)

    runs = rng.integers(8, 17, n // 8 + 1)
    doc_labels = np.repeat(np.arange(runs.size, dtype=np.uint32), runs)[:n]
    doc_rows = int(min(n, np.searchsorted(doc_labels, DOCS)))                    # the rows of the first DOCS documents
    layouts = (("documents", doc_labels, (0, 0, 0, 0, doc_rows - 1, 0, 0), doc_rows),
               ("random1000", rng.integers(0, 1000, n).astype(np.uint32), (0, 0, 0, I64_MIN, I64_MAX, 0, 0), n),
               ("one_label", np.zeros(n, np.uint32), (0, 0, 0, I64_MIN, I64_MAX, 0, 0), n))
    for name, labels, pred, considered in layouts:
        ix.set_labels(0, labels)
        groups_only = timed(lambda: ix.aggregate_where(pred, va.AGG_BY_LABEL, limit=0), a.warmup, a.calls)
        groups_all = timed(lambda: ix.aggregate_where(pred, va.AGG_BY_LABEL), a.warmup, a.calls)
        new = timed(lambda: ix.centroids_where(pred, va.AGG_BY_LABEL, capacity=va.MAX_CENTROID_GROUPS, out=out), a.warmup, a.calls)
        groups, vectors = new[2]
        rec = {"what": name, "rows": n, "considered": considered, "groups": int(groups.size), "ms_median": round(new[0], 4), "ms_min": round(new[1], 4),
               "aggregate_limit0_ms_median": round(groups_only[0], 4), "aggregate_all_ms_median": round(groups_all[0], 4),
               "row_bytes_per_s_TB": round(considered * DIM * 2 / (new[0] * 1e-3) / 1e12, 3)}
        assert int(groups["count"].sum()) == considered
        if a.host_route:
            def host_route():
                x = ix.get_rows(0, considered)
                lab = ix.get_labels(0, considered).astype(np.int64)
                order = np.argsort(lab, kind="stable")
                uniq, start = np.unique(lab[order], return_index=True)
                counts = np.diff(np.append(start, lab.size))
                return uniq, np.add.reduceat(x[order], start, axis=0, dtype=np.float64) / counts[:, None]
            old = timed(host_route, 0, a.host_calls)
            uniq, mean64 = old[2]
            got = vectors.cpu().numpy().astype(np.float64)
            a32 = np.abs(mean64).astype(np.float32)
            ulp = np.nextafter(a32, np.float32(np.inf)).astype(np.float64) - a32.astype(np.float64)
            assert np.array_equal(uniq, groups["key"]) and (np.abs(got - mean64) <= quantum + ulp).all()   # the same answer, within the bound
            rec.update({"host_route_ms_median": round(old[0], 1), "host_route_ms_min": round(old[1], 1), "ratio_host_over_new": round(old[0] / new[0], 1)})
        emit(rec)
    ix.close()


if __name__ == "__main__":
    main()
