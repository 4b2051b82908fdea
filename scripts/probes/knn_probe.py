"""What the exact k-NN graph costs: `--rows` x 768 bf16 cosine (synthetic rows), k = 10, the graph of the first
`--batches` x 1024 rows, three ways in one process over the same corpus:

  caller_loop   what a caller had to do before vrod_knn_graph existed: per batch of 1024 ids, vrod_index_get_rows (device
                -> host), vrod_search with k + 1 (host -> device, the rows prepared a second time), self dropped on the host;
  knn_graph     vrod_knn_graph over the same rows: gathered on the device, two batches in flight;
  pipelined     context, not a bar: vrod_search_begin_synthetic_device / vrod_search_end over as many batches of 1024 fresh
                synthetic queries, two in flight, results left on the device -- the scan pipeline with nothing around it.
Then, last, vrod_knn_graph once more with 5 % of the range's rows deleted (each batch's live rows compacted on the device).

Each is run `--repeats` times after one warm-up run; wall times, and ms per batch.  The caller's loop and the graph must
give the same neighbour ids (the scores may differ in bits: the loop's queries were prepared twice).  One JSON line per
measurement.

    python scripts/probes/knn_probe.py [--rows 1000000] [--batches 64] [--repeats 3]
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
BATCH = 1024


def caller_loop(ix, n, k):
    out = np.empty((n, k), np.uint64)
    for first in range(0, n, BATCH):
        m = min(BATCH, n - first)
        rows = ix.get_rows(first, m)
        ids, _ = ix.search(rows, k + 1)
        own = np.arange(first, first + m, dtype=np.uint64)[:, None]
        order = np.argsort(ids == own, axis=1, kind="stable")[:, :k]   # the entries that are not self, in list order
        out[first:first + m] = np.take_along_axis(ids, order, axis=1)
    return out


def pipelined(ix, n, k, bufs):
    nb = (n + BATCH - 1) // BATCH
    for b in range(nb):
        oi, osc = bufs[b & 1]
        ix.search_begin_synthetic_device(QUERY_SEED, b * BATCH, BATCH, k + 1, oi, osc)
        if b:
            ix.search_end()
    ix.search_end()


def timed(fn, repeats):
    fn()   # warm-up: workspaces grow, the candidate margin settles
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    n = min(a.batches * BATCH, a.rows)
    print(json.dumps({"probe": "knn", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(a.rows)
    ix.add_synthetic(CORPUS_SEED, 0, a.rows)
    nb = (n + BATCH - 1) // BATCH

    def report(what, times, extra):
        print(json.dumps({"what": what, "rows": n, "batches": nb, "wall_ms": [round(t, 3) for t in times], "wall_ms_min": round(min(times), 3),
                          "ms_per_batch_min": round(min(times) / nb, 4), **extra}), flush=True)

    t_loop, loop_ids = timed(lambda: caller_loop(ix, n, a.k), a.repeats)
    report("caller_loop", t_loop, {})
    t_graph, (g_ids, _) = timed(lambda: ix.knn_graph(a.k, first_id=0, n=n), a.repeats)
    st = ix.last_stats()
    report("knn_graph", t_graph, {"same_ids_as_loop": bool(np.array_equal(g_ids, loop_ids)), "path": st["path"], "scan_launches": st["scan_launches"],
                                  "fallback_queries": st["fallback_queries"], "band_queries": st["band_queries"]})
    bufs = [(torch.empty((BATCH, a.k + 1), dtype=torch.int64, device=dev), torch.empty((BATCH, a.k + 1), dtype=torch.float32, device=dev))
            for _ in range(2)]
    t_pipe, _ = timed(lambda: pipelined(ix, n, a.k, bufs), a.repeats)
    report("pipelined_synthetic", t_pipe, {})
    print(json.dumps({"what": "summary", "graph_over_loop": round(min(t_graph) / min(t_loop), 4),
                      "graph_over_pipelined": round(min(t_graph) / min(t_pipe), 4)}), flush=True)
    # last (it changes the corpus): the graph again with 5 % of the range deleted -- every batch is compacted on the device first
    dead = np.random.default_rng(3).choice(n, n // 20, replace=False)
    ix.delete(dead)
    t_del, (d_ids, _) = timed(lambda: ix.knn_graph(a.k, first_id=0, n=n), a.repeats)
    report("knn_graph_5pct_deleted", t_del, {"live_queries": ix.last_stats()["nq"], "deleted_rows_unfilled": bool((d_ids[dead] == va.ID_NONE).all())})
    ix.close()


if __name__ == "__main__":
    main()
