"""What a search with a tags + value-interval predicate costs: 10M x 768 bf16 cosine, batch 1024, k = 10.  The rows' tags
hold a 10-bit value t in bits 0 .. 9 (uniform: each on ~0.1 % of the rows); a row's value is 1000 * t + u, u uniform in
0 .. 999, so the window [1000 t, 1000 t + 999] holds exactly the rows whose tag value is t.

  (a) narrow   1024 distinct windows of ~0.1 % of the rows each, no tag clause;
  (b) wide     16 distinct windows of ~30 % of the rows, 64 queries each: the dense route, one masked scan per window;
  (c) as tags  the batch of (a) as tag predicates "the value is t" with the full interval, through search_where and
               through search_tagged: the same rows, so the difference is the wider predicate walk (40 B instead of 24 B
               per group from LDS, one more 8-byte load per row).

--tagged-only runs the search_tagged line of (c) alone and needs neither values nor search_where: the same script times
a build that predates them.  Median and minimum wall time per call, one JSON line per measurement; --repeats runs every
measurement again, so the spread between repeats is on record beside the result.

    python scripts/probes/where_probe.py [--rows 10000000] [--batches 7] [--warmup 2] [--repeats 3] [--tagged-only]
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
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


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


def tag_value_preds(values):
    """[n, 3] tag predicates "bits 0 .. 9 equal the value"."""
    v = np.asarray(values, dtype=np.uint64)
    p = np.zeros((v.size, 3), np.uint64)
    p[:, 1] = v
    p[:, 2] = ~v & VALUE_BITS
    return p


def where_preds(tag_preds, lo, hi):
    """[n, 5] int64: the tag predicates' bits, then the interval."""
    p = np.empty((len(lo), 5), np.int64)
    p[:, :3] = np.asarray(tag_preds, dtype=np.uint64).view(np.int64)
    p[:, 3], p[:, 4] = lo, hi
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tagged-only", action="store_true")
    a = ap.parse_args()
    print(json.dumps({"probe": "where", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(a.rows)
    ix.add_synthetic(CORPUS_SEED, 0, a.rows)
    dq = va.synth_rows_device(0, QUERY_SEED, 0, a.nq, a.dim)
    oi = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
    os_ = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
    tags = rng.integers(0, 1024, a.rows).astype(np.uint64)
    values = tags.astype(np.int64) * 1000 + rng.integers(0, 1000, a.rows)
    t0 = time.perf_counter()
    ix.set_tags(0, tags)
    print(json.dumps({"what": "set_tags", "rows": a.rows, "wall_s": round(time.perf_counter() - t0, 4)}), flush=True)
    if not a.tagged_only:
        t0 = time.perf_counter()
        ix.set_values(0, values)
        print(json.dumps({"what": "set_values", "rows": a.rows, "wall_s": round(time.perf_counter() - t0, 4)}), flush=True)
    ix.set_path(va.PATH_AUTO)

    def run(what, search, preds, repeat):
        dp = torch.from_numpy(np.ascontiguousarray(preds).view(np.int64)).to(dev)
        med, mn = timed(lambda b: search(dq, a.k, dp, oi, os_), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": what, "repeat": repeat, "distinct_predicates": int(np.unique(preds, axis=0).shape[0]),
                          "wall_ms_median": round(med, 4), "wall_ms_min": round(mn, 4), "path": st["path"], "scan_launches": st["scan_launches"],
                          "fallback_queries": st["fallback_queries"], "scan_bytes": st["scan_bytes"]}), flush=True)

    t = rng.permutation(1024)[np.arange(a.nq) % 1024]
    zeros = np.zeros((a.nq, 3), np.uint64)
    w = np.arange(a.nq) % 16
    for r in range(a.repeats):
        run("c_tag_predicates_search_tagged", ix.search_tagged_device, tag_value_preds(t), r)
        if a.tagged_only:
            continue
        run("c_tag_predicates_full_interval_search_where", ix.search_where_device,
            where_preds(tag_value_preds(t), np.full(a.nq, I64_MIN), np.full(a.nq, I64_MAX)), r)
        run("a_narrow_1024_windows_0p1pct_each", ix.search_where_device, where_preds(zeros, t * 1000, t * 1000 + 999), r)
        run("b_wide_16_windows_30pct_each", ix.search_where_device, where_preds(zeros, w * 45_000, w * 45_000 + 307_199), r)
    ix.close()


if __name__ == "__main__":
    main()
