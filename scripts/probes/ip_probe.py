"""What the inner-product metric costs against cosine, and how often a norm-skewed corpus sends queries to the band pass.

Part 1: a cosine handle and an IP handle over the same synthetic stream (unit rows, 10M x 768 bf16 by default); batches
of 1024 synthetic queries, k = 10, on each.  Part 2: the same two metrics over rows added through vrod_index_add, every
row of the stream scaled by exp(U(-1, 1)) (2M rows by default): the IP certificate's bound uses the corpus's LARGEST row
norm for every query, cosine normalises the skew away.  Prints one JSON line per handle: mean scan_ms / total_ms per
batch, mean fallback_queries and band_queries per batch.

    python scripts/probes/ip_probe.py [--rows 10000000] [--skew-rows 2000000] [--batches 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import vrod_amd as va  # noqa: E402

CORPUS_SEED, QUERY_SEED = 1, 2


def measure(ix, dim, nq, k, batches, warmup):
    dev = torch.device("cuda", 0)
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ix.set_profiling(2)
    rows = []
    for b in range(warmup + batches):
        ix.search_synthetic_device(QUERY_SEED, (b % 8) * nq, nq, k, oi, os_)
        torch.cuda.synchronize()
        if b >= warmup:
            rows.append(ix.last_stats())
    mean = lambda key: float(np.mean([r[key] for r in rows]))  # noqa: E731
    return {"scan_ms": round(mean("scan_ms"), 4), "total_ms": round(mean("total_ms"), 4),
            "fallback_queries": mean("fallback_queries"), "band_queries": mean("band_queries"),
            "kprime_last": rows[-1]["kprime"], "path": rows[-1]["path"], "eps_bound_last": rows[-1]["eps_bound"],
            "max_fast_err_last": rows[-1]["max_fast_err"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--skew-rows", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    box = {"device": torch.cuda.get_device_name(0), "library": va.version()}
    print(json.dumps({"probe": "ip", "box": box, "args": vars(a)}), flush=True)

    for metric in ("cosine", "ip"):
        with va.Index(a.dim, "bf16", metric) as ix:
            ix.reserve(a.rows)
            ix.add_synthetic(CORPUS_SEED, 0, a.rows)
            r = measure(ix, a.dim, a.nq, a.k, a.batches, a.warmup)
        print(json.dumps({"part": "unit", "rows": a.rows, "metric": metric, **r}), flush=True)

    # norm-skewed rows: the synthetic stream, each row scaled by exp(U(-1, 1)), added from the host in chunks
    rng = np.random.default_rng(5)
    scale = np.exp(rng.uniform(-1.0, 1.0, a.skew_rows)).astype(np.float32)
    for metric in ("cosine", "ip"):
        with va.Index(a.dim, "bf16", metric) as ix:
            ix.reserve(a.skew_rows)
            chunk = 1 << 17
            for lo in range(0, a.skew_rows, chunk):
                m = min(chunk, a.skew_rows - lo)
                rows = va.synth_rows_device(0, CORPUS_SEED, lo, m, a.dim)
                rows *= torch.from_numpy(scale[lo:lo + m]).to(rows.device)[:, None]
                ix.add(rows.cpu().numpy())
            r = measure(ix, a.dim, a.nq, a.k, a.batches, a.warmup)
        print(json.dumps({"part": "skewed", "rows": a.skew_rows, "metric": metric, **r}), flush=True)


if __name__ == "__main__":
    main()
