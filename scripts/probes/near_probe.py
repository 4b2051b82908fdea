"""What near-duplicate detection costs: 1M x 768 bf16 cosine handles, synthetic rows, with 0 % and 5 % of the rows made
near-copies of other rows -- the source row plus noise of a tenth of its norm (cosine about 0.995), far above the
threshold of 0.9 that no two independent synthetic rows reach.

Per handle, in one process:
  find_near_duplicates   wall time of the stats-only call, per call and per batch (stats["batches"] range scans);
  the yardstick          vrod_knn_graph (k = 10) over the first --knn-batches batches of the same handle, per batch: code
                         this feature does not touch.  ratio = near ms per batch / graph ms per batch;
  delete                 delete_near_duplicates, once, last (5 % handle only: it is a whole further call).
The 5 % result is checked before a time is reported: near_duplicates must equal the copies planted, and every copy's
class must be its source's.

    python scripts/probes/near_probe.py [--rows 1000000] [--repeats 2] [--knn-batches 16] > near_probe_1Mx768.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import vrod_amd as va  # noqa: E402
from vrod_amd._lib import NearStats, check  # noqa: E402

THRESHOLD = 0.9


def stats_only(ix, thr):
    st = NearStats()
    check(ix._L.vrod_index_find_near_duplicates(ix._h, thr, 0, None, 0, C.byref(st)))
    return st.as_dict()


def timed(fn, warmup, repeats):
    out, last = [], None
    for b in range(warmup + repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        if b >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return out, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--knn-batches", type=int, default=16)
    ap.add_argument("--fracs", type=float, nargs="*", default=[0.0, 0.05])
    a = ap.parse_args()

    def emit(rec):
        print(json.dumps(rec), flush=True)
    emit({"probe": "near", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a), "threshold": THRESHOLD})
    n, dim = a.rows, a.dim
    raw = va.synth_rows_device(0, 1, 0, n, dim)
    for frac in a.fracs:
        x = raw.clone()
        copies = int(n * frac)
        dst = src = None
        if copies:   # `copies` rows at shuffled positions become noisy copies of rows that stay as they are
            g = torch.Generator("cuda").manual_seed(7)
            perm = torch.randperm(n, device="cuda", generator=g)
            dst, src = perm[:copies], perm[copies:][torch.randint(0, n - copies, (copies,), device="cuda", generator=g)]
            noise = torch.randn((copies, dim), device="cuda", generator=g)
            noise *= 0.1 * x[src].norm(dim=1, keepdim=True) / noise.norm(dim=1, keepdim=True)
            x[dst] = x[src] + noise
        with va.Index(dim, "bf16", "cosine") as ix:
            ix.reserve(n)
            ix.add_device(x)
            del x
            batch = va.index.KNN_BATCH[va.DTYPE_BF16]
            ms, st = timed(lambda: stats_only(ix, THRESHOLD), a.warmup, a.repeats)
            assert st["rows"] == n and st["near_duplicates"] == copies and st["splits"] == 0, st
            if copies:   # every copy is in its source's class
                first = ix.find_near_duplicates(THRESHOLD)
                d, s = dst.cpu().numpy(), src.cpu().numpy()
                assert np.array_equal(first[d], first[s]) and np.all(first[d] <= np.minimum(d, s).astype(np.uint64))
            nb = min(a.knn_batches, -(-n // batch))
            knn_ms, _ = timed(lambda: ix.knn_graph(10, 0, nb * batch), a.warmup, a.repeats)
            rec = {"dtype": "bf16", "rows": n, "dim": dim, "planted_near_copies": copies, "stats": st,
                   "find_stats_only_ms": {"runs": ms, "min": min(ms)}, "near_ms_per_batch": min(ms) / st["batches"],
                   "knn_graph": {"k": 10, "batches": nb, "runs_ms": knn_ms, "min_ms": min(knn_ms), "ms_per_batch": min(knn_ms) / nb}}
            rec["near_over_knn_per_batch"] = rec["near_ms_per_batch"] / rec["knn_graph"]["ms_per_batch"]
            if copies:
                torch.cuda.synchronize()
                t = time.perf_counter()
                died = ix.delete_near_duplicates(THRESHOLD)
                rec["delete_near_duplicates_ms"] = (time.perf_counter() - t) * 1e3
                assert died == copies and ix.live_count() == n - copies
            emit(rec)


if __name__ == "__main__":
    main()
