"""What a tagged search costs: 10M x 768 bf16 cosine, batch 1024, k = 10.  The rows' tags hold a 10-bit value in bits
0 .. 9 (uniform: each value on ~0.1 % of the rows) and bit 63 on half of the rows; bit 62 is on no row.

  count pass   a tagged search with 1, 64 and 1024 distinct predicates that no row matches (each asks for bit 62 too):
               query preparation, the count pass over the 80 MB tag array, the prefix, one select over empty segments, no
               score launch -- the counterpart of label_probe.py's "grouping_only" line;
  narrow       1024 distinct predicates "the value is v" (all of v's ones, none of its zeros), ~0.1 % of the rows each;
  wide         one predicate on bit 63 for the whole batch (50 % of the rows: one masked scan).

Median and minimum wall time of vrod_search_tagged_device, one JSON line per measurement.

    python scripts/probes/tag_probe.py [--rows 10000000] [--batches 7] [--warmup 2]
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

CORPUS_SEED, QUERY_SEED = 1, 2
VALUE_BITS = np.uint64(0x3FF)
ABSENT = np.uint64(1) << np.uint64(62)


def timed(fn, warmup, batches):
    out = []
    for b in range(warmup + batches):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(b)
        torch.cuda.synchronize()
        if b >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out))


def value_preds(values, extra_all=np.uint64(0)):
    """[n, 3] predicates "bits 0 .. 9 equal the value" (and carry `extra_all`)."""
    v = np.asarray(values, dtype=np.uint64)
    p = np.zeros((v.size, 3), np.uint64)
    p[:, 1] = v | extra_all
    p[:, 2] = ~v & VALUE_BITS
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    print(json.dumps({"probe": "tag", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(a.rows)
    ix.add_synthetic(CORPUS_SEED, 0, a.rows)
    dq = va.synth_rows_device(0, QUERY_SEED, 0, a.nq, a.dim)
    oi = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
    os_ = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
    tags = rng.integers(0, 1024, a.rows).astype(np.uint64)
    tags[rng.random(a.rows) < 0.5] |= np.uint64(1) << np.uint64(63)
    t0 = time.perf_counter()
    ix.set_tags(0, tags)
    print(json.dumps({"what": "set_tags", "rows": a.rows, "wall_s": round(time.perf_counter() - t0, 4)}), flush=True)
    ix.set_path(va.PATH_AUTO)

    def run(what, preds, **more):
        dp = torch.from_numpy(np.ascontiguousarray(preds).view(np.int64)).to(dev)
        med, mn = timed(lambda b: ix.search_tagged_device(dq, a.k, dp, oi, os_), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": what, "distinct_predicates": int(np.unique(preds, axis=0).shape[0]), "wall_ms_median": round(med, 4),
                          "wall_ms_min": round(mn, 4), "path": st["path"], "scan_launches": st["scan_launches"],
                          "fallback_queries": st["fallback_queries"], "scan_bytes": st["scan_bytes"], **more}), flush=True)

    for g in (1, 64, 1024):
        run("count_pass_only_no_row_matches", value_preds(np.arange(a.nq) % g, ABSENT))
    run("narrow_1024_predicates_0p1pct_each", value_preds(rng.permutation(1024)[np.arange(a.nq) % 1024]))
    run("wide_one_predicate_50pct", np.tile(np.array([[np.uint64(1) << np.uint64(63), 0, 0]], np.uint64), (a.nq, 1)))
    ix.close()


if __name__ == "__main__":
    main()
