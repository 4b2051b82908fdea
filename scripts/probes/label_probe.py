"""What a mixed-tenant batch costs: 10M x 768 bf16 cosine, batch 1024, k = 10, with the rows labelled by tenant in three
layouts -- 1000 uniform tenants (0.1 % of the rows each), 16 uniform tenants, and a skewed one (one tenant on 50 % of
the rows, the rest in tenants of 0.05 % each) -- and every query drawn from a tenant in proportion to its rows.

Per layout: the median wall time of vrod_search_labeled_device (one call for the whole batch), and beside it the time
of what a caller does without labels: per distinct tenant of the batch, set_filter(rows of the tenant) + a search of
that tenant's queries.  The loop is timed over --loop-labels tenants of the batch (all of them when 0) and scaled to
the batch's distinct tenants; the filter bitmaps are built before the clock starts.  Also: the grouping pass alone
(a labelled search whose queries all ask for a label no row carries scores nothing: prepare + one pass over the label
array + one select of empty segments).  One JSON line per measurement.

    python scripts/probes/label_probe.py [--rows 10000000] [--batches 7] [--warmup 2] [--loop-labels 24]
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


def layouts(n, rng):
    yield "uniform_1000", rng.integers(0, 1000, n).astype(np.uint32)
    yield "uniform_16", rng.integers(0, 16, n).astype(np.uint32)
    lab = rng.integers(1, 1001, n).astype(np.uint32)        # 1000 tenants of 0.05 % on one half ...
    lab[rng.random(n) < 0.5] = 0                            # ... tenant 0 on the other
    yield "skewed", lab


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-labels", type=int, default=24)
    a = ap.parse_args()
    print(json.dumps({"probe": "label", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(a.rows)
    ix.add_synthetic(CORPUS_SEED, 0, a.rows)
    dq = va.synth_rows_device(0, QUERY_SEED, 0, a.nq, a.dim)
    oi = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
    os_ = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
    for name, lab in layouts(a.rows, rng):
        t0 = time.perf_counter()
        ix.set_labels(0, lab)
        set_s = time.perf_counter() - t0
        ql = lab[rng.integers(0, a.rows, a.nq)]             # a tenant in proportion to its rows
        dl = torch.from_numpy(ql.view(np.int32)).to(dev)
        distinct = np.unique(ql)
        ix.set_filter(None)
        ix.set_path(va.PATH_AUTO)
        med, mn = timed(lambda b: ix.search_labeled_device(dq, a.k, dl, oi, os_), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"layout": name, "what": "search_labeled", "distinct_labels": int(distinct.size), "wall_ms_median": round(med, 4),
                          "wall_ms_min": round(mn, 4), "path": st["path"], "scan_launches": st["scan_launches"],
                          "fallback_queries": st["fallback_queries"], "set_labels_s": round(set_s, 4)}), flush=True)
        # the grouping pass alone: 1024 queries for a label no row carries
        dn = torch.full((a.nq,), 0x7FFFFFF0, dtype=torch.int32, device=dev)
        med, mn = timed(lambda b: ix.search_labeled_device(dq, a.k, dn, oi, os_), a.warmup, a.batches)
        print(json.dumps({"layout": name, "what": "grouping_only_one_absent_label", "wall_ms_median": round(med, 4), "wall_ms_min": round(mn, 4)}), flush=True)
        # the caller's loop without labels: set_filter + search per distinct tenant of the batch
        pick = distinct if not a.loop_labels else distinct[np.argsort([-(ql == L).sum() for L in distinct], kind="stable")][:a.loop_labels]
        sets, searches, routes = [], [], {}
        for L in pick:
            allow = lab == L
            qs = torch.from_numpy(np.flatnonzero(ql == L)).to(dev)
            dqg = dq[qs].contiguous()
            torch.cuda.synchronize()
            t = time.perf_counter()
            ix.set_filter(allow)
            t1 = time.perf_counter()
            ix.search_device(dqg, a.k)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            sets.append((t1 - t) * 1e3)
            searches.append((t2 - t1) * 1e3)
            p = ix.last_stats()["path"]
            routes[p] = routes.get(p, 0) + 1
        ix.set_filter(None)
        per = float(np.mean(sets)) + float(np.mean(searches))
        print(json.dumps({"layout": name, "what": "set_filter_search_loop", "labels_timed": int(len(pick)), "distinct_labels": int(distinct.size),
                          "set_filter_ms_mean": round(float(np.mean(sets)), 3), "search_ms_mean": round(float(np.mean(searches)), 3),
                          "loop_ms_timed": round(float(np.sum(sets) + np.sum(searches)), 3),
                          "loop_ms_scaled_to_batch": round(per * distinct.size, 3), "paths": routes}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
