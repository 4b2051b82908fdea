"""What a search by weighted examples costs over the search it stands on: bf16 cosine synthetic rows (the benchmark's
generator, built on the device), the _device form with every pointer resident, median wall time after a warm-up.

Per shape a pair on one handle:
  combined      vrod_search_combined_device(nq, k, 8 terms per query, E excluded ids per query), no vector operand;
  search_at_k1  vrod_search_device of nq synthetic queries at k = k1 = k + E: the unchanged plain search, the baseline.  The
                difference is the combine launch with its flag read-back, the copy of the lims arrays to the host and --
                with E > 0 -- the drop launch.
Shapes: nq = 1024 and nq = 1, k = 10, 8 terms, E = 0 and E = 100 (the excluded ids are the query's own best 100 rows of
an unexcluded call: every one of them is dropped).  One JSON line per measurement.

    python scripts/probes/combine_probe.py [--rows 1000000] [--batches 5] [--warmup 1]
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
    ap.add_argument("--terms", type=int, default=8)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps({"probe": "combine", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    ix = va.Index(a.dim, "bf16", "cosine")
    t0 = time.perf_counter()
    ix.add_synthetic(1, 0, a.rows)
    print(json.dumps({"what": "corpus", "rows": a.rows, "dim": a.dim, "build_s": round(time.perf_counter() - t0, 2)}), flush=True)
    g = torch.Generator(device="cpu").manual_seed(3)
    k = 10
    for nq in (1024, 1):
        lims = (torch.arange(nq + 1, dtype=torch.int32) * a.terms).to(dev)
        ids = torch.randint(0, a.rows, (nq * a.terms,), generator=g, dtype=torch.int64).to(dev)
        w = (torch.rand(nq * a.terms, generator=g) * 2 - 1).to(dev)
        dq = va.synth_rows_device(0, 2, 0, nq, a.dim)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
        for E in (0, 100):
            k1 = k + E
            xl = xi = None
            if E:   # each query's own best E rows, from an unexcluded call
                bi = torch.empty((nq, E), dtype=torch.int64, device=dev)
                bs = torch.empty((nq, E), dtype=torch.float32, device=dev)
                ix.search_combined_device(E, lims, ids, w, out_ids=bi, out_scores=bs)
                xl = (torch.arange(nq + 1, dtype=torch.int32) * E).to(dev)
                xi = bi.reshape(-1).contiguous()
            c_med, c_min = timed(lambda: ix.search_combined_device(k, lims, ids, w, d_exclude_lims=xl, d_exclude_ids=xi, out_ids=oi, out_scores=os_),
                                 a.warmup, a.batches)
            st = ix.last_stats()
            print(json.dumps({"what": "combined", "nq": nq, "k": k, "terms": a.terms, "excluded": E, "k1": k1, "wall_ms_median": round(c_med, 3),
                              "wall_ms_min": round(c_min, 3), "path": st["path"], "fallback_queries": st["fallback_queries"]}), flush=True)
            if E:
                print(json.dumps({"what": "every_excluded_id_is_gone", "nq": nq, "ok": not bool((oi.unsqueeze(2) == bi.unsqueeze(1)).any())}), flush=True)
            pi = torch.empty((nq, k1), dtype=torch.int64, device=dev)
            ps = torch.empty((nq, k1), dtype=torch.float32, device=dev)
            f_med, f_min = timed(lambda: ix.search_device(dq, k1, pi, ps), a.warmup, a.batches)
            st = ix.last_stats()
            print(json.dumps({"what": "search_at_k1", "nq": nq, "k": k1, "wall_ms_median": round(f_med, 3), "wall_ms_min": round(f_min, 3),
                              "path": st["path"], "fallback_queries": st["fallback_queries"]}), flush=True)
            print(json.dumps({"what": "combined_adds", "nq": nq, "excluded": E, "ms": round(c_med - f_med, 3),
                              "over_baseline": round((c_med - f_med) / f_med, 3)}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
