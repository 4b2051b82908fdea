"""What a diversified search costs over the search it stands on: bf16 cosine synthetic rows (the benchmark's generator,
built on the device), synthetic queries, the _device form with every pointer resident, median wall time after a warm-up.

Two shapes, each as a pair:
  diverse          vrod_search_diverse_device(nq, k, pool, lambda);
  search_at_pool   vrod_search_device of the same queries at k = pool on the same handle: the floor -- the first stage is
                   this very search, so the difference is the selection launch (and its one synchronisation).
Shapes: nq = 1024, k = 10, pool = 100 (the serving case), and nq = 1, k = 100, pool = 1024 (the worst serial case: one
work-group, 100 dependent rounds).  A last line checks lambda = 1 against the floor's first k, bit for bit.  One JSON
line per measurement.

    python scripts/probes/diverse_probe.py [--rows 1000000] [--batches 5] [--warmup 1]
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


def timed(fn, warmup, batches):
    out = []
    for b in range(warmup + batches):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if b >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps({"probe": "diverse", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    ix = va.Index(a.dim, "bf16", "cosine")
    t0 = time.perf_counter()
    ix.add_synthetic(1, 0, a.rows)
    print(json.dumps({"what": "corpus", "rows": a.rows, "dim": a.dim, "build_s": round(time.perf_counter() - t0, 2)}), flush=True)
    for nq, k, pool in ((1024, 10, 100), (1, 100, 1024)):
        dq = va.synth_rows_device(0, 2, 0, nq, a.dim)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
        om = torch.empty((nq, k), dtype=torch.float32, device=dev)
        pi = torch.empty((nq, pool), dtype=torch.int64, device=dev)
        ps = torch.empty((nq, pool), dtype=torch.float32, device=dev)
        d_med, d_min = timed(lambda: ix.search_diverse_device(dq, k, pool, a.lam, oi, os_, om), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": "diverse", "nq": nq, "k": k, "pool": pool, "lambda": a.lam, "wall_ms_median": round(d_med, 3),
                          "wall_ms_min": round(d_min, 3), "path": st["path"], "fallback_queries": st["fallback_queries"]}), flush=True)
        f_med, f_min = timed(lambda: ix.search_device(dq, pool, pi, ps), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": "search_at_pool", "nq": nq, "k": pool, "wall_ms_median": round(f_med, 3), "wall_ms_min": round(f_min, 3),
                          "path": st["path"], "fallback_queries": st["fallback_queries"]}), flush=True)
        moved = float((oi != pi[:, :k]).any(dim=1).float().mean())
        print(json.dumps({"what": "selection_adds", "nq": nq, "k": k, "pool": pool, "ms": round(d_med - f_med, 3),
                          "over_floor": round((d_med - f_med) / f_med, 3), "queries_reordered": round(moved, 3)}), flush=True)
        ix.search_diverse_device(dq, k, pool, 1.0, oi, os_, om)
        same = bool(torch.equal(oi, pi[:, :k]) and torch.equal(os_.view(torch.int32), ps[:, :k].contiguous().view(torch.int32)))
        print(json.dumps({"what": "lambda_one_is_the_floor", "nq": nq, "k": k, "pool": pool, "same_bits": same}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
