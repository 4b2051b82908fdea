"""What deleted rows cost the batched scan: cfg3 (10M x 768 bf16 cosine, batch 1024, k = 10) on a handle with 10 % of
its rows deleted at random against the same corpus with none deleted.

Two handles over the same synthetic stream; batches of synthetic queries alternate between them, so that clock and
thermal drift hit both alike.  Per handle: the median wall time of a synchronous search (vrod_search_synthetic_device),
the mean scan_ms / sample_ms of the library's own events (a second run with profiling on), fallback and band queries.
Prints one JSON line per handle and one with the ratio.

    python scripts/probes/delete_probe.py [--rows 10000000] [--frac 0.1] [--batches 30] [--warmup 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--frac", type=float, default=0.1, help="share of the rows deleted on the second handle")
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps({"probe": "delete", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    oi = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
    os_ = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
    handles = {}
    for name in ("none", "deleted"):
        ix = va.Index(a.dim, "bf16", "cosine")
        ix.reserve(a.rows)
        ix.add_synthetic(CORPUS_SEED, 0, a.rows)
        handles[name] = ix
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    handles["deleted"].delete(rng.choice(a.rows, int(a.rows * a.frac), replace=False))
    delete_s = time.perf_counter() - t0

    def run(profiling):
        wall = {n: [] for n in handles}
        stats = {n: [] for n in handles}
        for ix in handles.values():
            ix.set_profiling(profiling)
        for b in range(a.warmup + a.batches):
            for n, ix in (handles.items() if b % 2 == 0 else reversed(list(handles.items()))):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ix.search_synthetic_device(QUERY_SEED, (b % 8) * a.nq, a.nq, a.k, oi, os_)
                torch.cuda.synchronize()
                if b >= a.warmup:
                    wall[n].append((time.perf_counter() - t) * 1e3)
                    stats[n].append(ix.last_stats())
        return wall, stats

    wall, _ = run(0)
    _, stats = run(1)
    out = {}
    for n in handles:
        mean = lambda key: float(np.mean([r[key] for r in stats[n]]))  # noqa: E731
        out[n] = {"handle": n, "live_rows": handles[n].live_count(), "wall_ms_median": round(float(np.median(wall[n])), 4),
                  "wall_ms_min": round(float(np.min(wall[n])), 4), "scan_ms": round(mean("scan_ms"), 4),
                  "sample_ms": round(mean("sample_ms"), 4), "scan_launches": mean("scan_launches"),
                  "fallback_queries": mean("fallback_queries"), "band_queries": mean("band_queries"),
                  "kprime_last": stats[n][-1]["kprime"]}
        print(json.dumps(out[n]), flush=True)
    print(json.dumps({"ratio_wall_median": round(out["deleted"]["wall_ms_median"] / out["none"]["wall_ms_median"], 4),
                      "ratio_scan_ms": round(out["deleted"]["scan_ms"] / out["none"]["scan_ms"], 4),
                      "delete_call_s": round(delete_s, 4)}), flush=True)
    for ix in handles.values():
        ix.close()


if __name__ == "__main__":
    main()
