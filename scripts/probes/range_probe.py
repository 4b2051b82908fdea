"""What a range search costs against the top-k search of the same batch: 10M x 768 bf16 cosine, batch 1024, synthetic
streams 1 (corpus) / 2 (queries).

Baseline: vrod_search_device at k = 10 (the cfg3 shape), taken twice -- the spread between the two repeats is the noise
figure.  Then vrod_range_search_device with per-query thresholds at each query's 10th-, 1000th- and ~20000th-best score
(taken from top-k results of the same handle; the last one is estimated from the 3584th-best by the tail's slope, so
"~"): rows returned, scan_launches (more than 1: lists overflowed and the range was redone in pieces), scan_ms and
total_ms from the library's stats, and the median wall time of the synchronous call.  One JSON line per run.

VROD_HIP_LIB points the same script at another build of the library (a parent build has no range search: only the
baseline lines are printed).

--check compares every range result (lims, ids, score bits) with oracle.range_search over the same synthetic rows,
in blocks of a million rows on the host: meant for --rows of a few million at most.

    python scripts/probes/range_probe.py [--rows 10000000] [--batches 10] [--warmup 2] [--check]
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


def oracle_check(a, dq, thr, lims, ids, sc):
    """The device result against oracle.range_search (bf16, cosine), the corpus scanned in row blocks and merged."""
    from oracle import oracle as O
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    rq = O.synth_rows(QUERY_SEED, 0, a.nq, a.dim, threads=threads)
    assert np.array_equal(rq.view(np.uint32), dq.cpu().numpy().view(np.uint32))
    h_thr = thr.cpu().numpy()
    parts = [O.range_search(O.synth_rows(CORPUS_SEED, lo, min(10 ** 6, a.rows - lo), a.dim, threads=threads), rq, h_thr, O.DTYPE_BF16,
                            O.METRIC_COSINE, O.METRIC_COSINE, id_offset=lo, threads=threads) for lo in range(0, a.rows, 10 ** 6)]
    ol, oi, osc = O.merge_range(parts, O.METRIC_COSINE)
    total = int(ol[-1])
    return bool(np.array_equal(lims.cpu().numpy().view(np.uint64), ol) and np.array_equal(ids.cpu().numpy().view(np.uint64)[:total], oi)
                and np.array_equal(sc.cpu().numpy()[:total].view(np.uint32), osc.view(np.uint32)))


def timed(fn, batches, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(batches):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true", help="compare every range result with oracle.range_search")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    has_range = hasattr(va.load(), "vrod_range_search_device")
    with va.Index(a.dim, "bf16", "cosine") as ix:
        ix.add_synthetic(CORPUS_SEED, 0, a.rows)
        ix.set_profiling(2)
        dq = va.synth_rows_device(0, QUERY_SEED, 0, a.nq, a.dim)
        oi = torch.empty((a.nq, 10), dtype=torch.int64, device=dev)
        osc = torch.empty((a.nq, 10), dtype=torch.float32, device=dev)
        base = []
        for rep in range(2):
            med, best = timed(lambda: ix.search_device(dq, 10, oi, osc), a.batches, a.warmup)
            st = ix.last_stats()
            base.append(med)
            print(json.dumps({"run": "topk10", "repeat": rep, "median_ms": med, "min_ms": best, "scan_ms": st["scan_ms"], "total_ms": st["total_ms"],
                              "scan_launches": st["scan_launches"], "kprime": st["kprime"], "lib": va.version()}), flush=True)
        print(json.dumps({"run": "topk10_spread", "ms": abs(base[0] - base[1]), "relative": abs(base[0] - base[1]) / min(base)}), flush=True)
        if not has_range:
            return
        kbig = min(va.MAX_K, a.rows)
        bi = torch.empty((a.nq, kbig), dtype=torch.int64, device=dev)
        bs = torch.empty((a.nq, kbig), dtype=torch.float32, device=dev)
        ix.search_device(dq, kbig, bi, bs)
        s10, s1000, slast = osc[:, 9].clone(), bs[:, min(999, kbig - 1)].clone(), bs[:, kbig - 1].clone()
        # ~20000th best: the tail of the score distribution is close to linear in log(rank) over this span
        slope = (slast - s1000) / (np.log(kbig) - np.log(1000.0))
        s20000 = slast + slope * (np.log(20000.0) - np.log(kbig))
        for name, thr in (("range@10th", s10), ("range@1000th", s1000), ("range@~20000th", s20000)):
            thr = thr.contiguous()
            rc, lims, _, _ = ix.range_search_device(dq, thr, 0)
            total = int(lims[-1].item())
            ids = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            sc = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
            state = {}

            def run():
                state["rc"] = ix.range_search_device(dq, thr, total, lims, ids, sc)[0]
            med, best = timed(run, max(3, a.batches // (1 if total < 10 ** 6 else 3)), a.warmup)
            st = ix.last_stats()
            per = torch.diff(lims).cpu().numpy()
            extra = {"oracle_equal": oracle_check(a, dq, thr, lims, ids, sc)} if a.check else {}
            print(json.dumps({**extra, "run": name, "rc": state["rc"], "rows_total": total, "rows_per_query_min": int(per.min()), "rows_per_query_max": int(per.max()),
                              "median_ms": med, "min_ms": best, "scan_ms": st["scan_ms"], "total_ms": st["total_ms"], "scan_launches": st["scan_launches"],
                              "kprime": st["kprime"], "fallback_queries": st["fallback_queries"], "max_fast_err": st["max_fast_err"],
                              "eps_bound": st["eps_bound"], "vs_topk10": med / min(base)}), flush=True)


if __name__ == "__main__":
    main()
