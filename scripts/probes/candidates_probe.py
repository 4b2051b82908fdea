"""What a candidate-list search costs beside the full search of the same batch: bf16 cosine synthetic rows (the benchmark's
generator, built on the device), the _device forms with every pointer resident, median wall time after a warm-up.

Per list length L on one handle:
  search_candidates  vrod_search_candidates_device(nq, k, L random ids per query).  scan_ms (profiling level 1: events around
                     the score launches) is the score step; wall - scan_ms is everything else: the copy of the lims array
                     to the host, resolve, sort + unique, the read-back of the lengths, the select chain and the output;
  score_candidates   vrod_score_candidates_device of the same lists: resolve and ONE chain launch, no sort and no select;
  full_search        vrod_search_device of the same queries over the whole corpus: the yardstick, the unchanged plain search.
The split of the device time by kernel (resolve / sort / score / select) comes from running this script under
`rocprofv3 --kernel-trace --stats`; the kernels are cand_resolve_kernel, cand_sort_unique_kernel, rescore_segments_kernel,
select_chunk_kernel + seg_keys_to_output_kernel, and cand_score_kernel for the score form.  One JSON line per measurement.

    python scripts/probes/candidates_probe.py [--rows 1000000] [--nq 1024] [--batches 5] [--warmup 1]
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
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lengths", type=int, nargs="+", default=[100, 1000, 16384])
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    print(json.dumps({"probe": "candidates", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    ix = va.Index(a.dim, "bf16", "cosine")
    t0 = time.perf_counter()
    ix.add_synthetic(1, 0, a.rows)
    print(json.dumps({"what": "corpus", "rows": a.rows, "dim": a.dim, "build_s": round(time.perf_counter() - t0, 2)}), flush=True)
    ix.set_profiling(1)
    g = torch.Generator(device="cpu").manual_seed(3)
    nq, k = a.nq, a.k
    dq = va.synth_rows_device(0, 2, 0, nq, a.dim)
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    os_ = torch.empty((nq, k), dtype=torch.float32, device=dev)
    f_med, f_min = timed(lambda: ix.search_device(dq, k, oi, os_), a.warmup, a.batches)
    st = ix.last_stats()
    print(json.dumps({"what": "full_search", "nq": nq, "k": k, "wall_ms_median": round(f_med, 3), "wall_ms_min": round(f_min, 3), "path": st["path"],
                      "scan_ms": round(st["scan_ms"], 3), "fallback_queries": st["fallback_queries"]}), flush=True)
    full_ids = oi.clone()
    for L in a.lengths:
        lims = (torch.arange(nq + 1, dtype=torch.int64) * L).to(torch.int32).to(dev)
        ids = torch.randint(0, a.rows, (nq * L,), generator=g, dtype=torch.int64)
        ids[::L] = full_ids[:, 0].cpu()   # every list holds its query's best row: the result's first slot is known
        ids = ids.to(dev)
        fs = torch.empty(nq * L, dtype=torch.float32, device=dev)
        c_med, c_min = timed(lambda: ix.search_candidates_device(dq, k, lims, ids, out_ids=oi, out_scores=os_), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": "search_candidates", "nq": nq, "k": k, "list": L, "wall_ms_median": round(c_med, 3), "wall_ms_min": round(c_min, 3),
                          "score_ms": round(st["scan_ms"], 3), "other_ms": round(c_med - st["scan_ms"], 3), "score_launches": st["scan_launches"],
                          "kprime": st["kprime"], "rows_scored": st["scan_flops"] / (2.0 * a.dim), "of_full_search": round(c_med / f_med, 3),
                          "first_slot_is_the_full_search_best": bool((oi[:, 0] == full_ids[:, 0]).all())}), flush=True)
        s_med, s_min = timed(lambda: ix.score_candidates_device(dq, lims, ids, out_scores=fs), a.warmup, a.batches)
        st = ix.last_stats()
        print(json.dumps({"what": "score_candidates", "nq": nq, "list": L, "wall_ms_median": round(s_med, 3), "wall_ms_min": round(s_min, 3),
                          "score_ms": round(st["scan_ms"], 3), "other_ms": round(s_med - st["scan_ms"], 3), "rows_scored": st["scan_flops"] / (2.0 * a.dim),
                          "of_full_search": round(s_med / f_med, 3), "nan_scores": int(torch.isnan(fs).sum())}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
