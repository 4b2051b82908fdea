"""What an allow-list filter costs: 10M x 768 bf16 cosine, k = 10, batches of 1024 and 4 synthetic queries, with 100 /
50 / 10 / 1 / 0.1 / 0.01 % of the rows allowed at random -- the dense path forced (MFMA for the batch of 1024, stream
for 4), the gather path forced, and AUTO.

Per (fraction, batch, mode): the median wall time of a synchronous search (vrod_search_synthetic_device), the path
taken, failed certificates and band-pass queries per batch, and the time of the first search after set_filter (the
gather path builds its row list then).  Forced gather runs whose estimate (search_plan.h filter_cost) exceeds
--max-gather-ms are skipped.  The gather kernel's rate -- canonical chain steps (query x row x element) per second --
is printed per run: it sets kGatherNsPerStep of search_plan.h.  One JSON line per run.

    python scripts/probes/filter_probe.py [--rows 10000000] [--batches 10] [--warmup 2]
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
FRACS = [1.0, 0.5, 0.1, 0.01, 0.001, 0.0001]


def est_gather_ms(m, nq, dim):
    # search_plan.h filter_cost, gather side (bf16 rows)
    return m * (dim * 2 * 3.0e-4 + nq * dim * 1.56e-4) * 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nqs", default="1024,4")
    ap.add_argument("--fracs", default=",".join(str(f) for f in FRACS))
    ap.add_argument("--max-gather-ms", type=float, default=400.0)
    a = ap.parse_args()
    print(json.dumps({"probe": "filter", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    nqs = [int(x) for x in a.nqs.split(",")]
    fracs = [float(x) for x in a.fracs.split(",")]
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(a.rows)
    ix.add_synthetic(CORPUS_SEED, 0, a.rows)
    rng = np.random.default_rng(7)
    u = rng.random(a.rows)
    for frac in fracs:
        t0 = time.perf_counter()
        ix.set_filter(None if frac >= 1.0 else u < frac)
        set_s = time.perf_counter() - t0
        m = ix.filter_count()
        for nq in nqs:
            oi = torch.empty((nq, a.k), dtype=torch.int64, device=dev)
            os_ = torch.empty((nq, a.k), dtype=torch.float32, device=dev)
            dense = va.PATH_MFMA if nq > 4 else va.PATH_STREAM
            for mode, path in (("dense", dense), ("gather", va.PATH_GATHER), ("auto", va.PATH_AUTO)):
                if mode == "gather" and est_gather_ms(m, nq, a.dim) > a.max_gather_ms:
                    print(json.dumps({"frac": frac, "nq": nq, "mode": mode, "skipped": f"estimate {est_gather_ms(m, nq, a.dim):.0f} ms"}), flush=True)
                    continue
                ix.set_path(path)
                wall, stats, first_ms = [], [], None
                for b in range(a.warmup + a.batches):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    ix.search_synthetic_device(QUERY_SEED, (b % 8) * nq, nq, a.k, oi, os_)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t) * 1e3
                    if first_ms is None:
                        first_ms = ms
                    if b >= a.warmup:
                        wall.append(ms)
                        stats.append(ix.last_stats())
                med = float(np.median(wall))
                rec = {"frac": frac, "nq": nq, "mode": mode, "eligible": m, "path": stats[-1]["path"],
                       "wall_ms_median": round(med, 4), "wall_ms_min": round(float(np.min(wall)), 4),
                       "first_ms": round(first_ms, 4), "fallback_per_batch": float(np.mean([s["fallback_queries"] for s in stats])),
                       "band_per_batch": float(np.mean([s["band_queries"] for s in stats])), "set_filter_s": round(set_s, 4)}
                if stats[-1]["path"] == va.PATH_GATHER and m:
                    rec["gather_steps_per_s"] = float(nq) * m * a.dim / (med * 1e-3)
                print(json.dumps(rec), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
