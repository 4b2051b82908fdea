"""What a grouped search costs: 10M x 768 bf16 cosine, k = 10, rows labelled as documents of `--chunks` consecutive rows
(random synthetic rows: the best ranks of a query belong to different documents, so the candidate search resolves every
query).

Per batch size: the median wall time of vrod_search_grouped_device beside vrod_search_device at the same k1 =
max(4 k, k + 32) -- the grouped search minus the plain one is the de-duplication and its read-back.  Then the dense
stage alone: set_path(PATH_EXACT) sends every query to it; 8 queries are one pass over the corpus (canonical scores of
every row), one mask / select / de-duplicate round, and a second round only for queries the first left unresolved.
One JSON line per measurement.

    python scripts/probes/group_probe.py [--rows 10000000] [--batches 7] [--warmup 2]
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
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    print(json.dumps({"probe": "group", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(a.rows)
    ix.add_synthetic(CORPUS_SEED, 0, a.rows)
    ix.set_labels(0, (np.arange(a.rows, dtype=np.uint64) // a.chunks).astype(np.uint32))
    k1 = max(4 * a.k, a.k + 32)
    for nq in (1, 8, 64, 1024):
        dq = va.synth_rows_device(0, QUERY_SEED, 0, nq, a.dim)
        gi = torch.empty((nq, a.k), dtype=torch.int64, device=dev)
        gs = torch.empty((nq, a.k), dtype=torch.float32, device=dev)
        gl = torch.empty((nq, a.k), dtype=torch.int32, device=dev)
        pi = torch.empty((nq, k1), dtype=torch.int64, device=dev)
        ps = torch.empty((nq, k1), dtype=torch.float32, device=dev)
        ix.set_path(va.PATH_AUTO)
        med, mn = timed(lambda b: ix.search_grouped_device(dq, a.k, gi, gs, gl), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": "search_grouped", "nq": nq, "k": a.k, "k1": k1, "wall_ms_median": round(med, 4), "wall_ms_min": round(mn, 4),
                          "path": st["path"], "fallback_queries": st["fallback_queries"]}), flush=True)
        med, mn = timed(lambda b: ix.search_device(dq, k1, pi, ps), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": "search_at_k1", "nq": nq, "k": k1, "wall_ms_median": round(med, 4), "wall_ms_min": round(mn, 4),
                          "path": st["path"], "fallback_queries": st["fallback_queries"]}), flush=True)
    dq = va.synth_rows_device(0, QUERY_SEED, 0, 8, a.dim)
    ix.set_path(va.PATH_EXACT)
    med, mn = timed(lambda b: ix.search_grouped_device(dq, a.k), a.warmup, a.batches)
    st = ix.last_stats()
    print(json.dumps({"what": "dense_stage_8_queries", "k": a.k, "wall_ms_median": round(med, 4), "wall_ms_min": round(mn, 4),
                      "path": st["path"], "fallback_queries": st["fallback_queries"], "scan_bytes": st["scan_bytes"]}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
