"""What compaction and in-place update cost, and what compaction buys: cfg3 (10M x 768 bf16 cosine, batch 1024, k = 10).

Per deletion pattern (10 % and 50 % at random, a deleted 30 % prefix) on a fresh handle over the synthetic stream:
  - the median wall time of a synchronous search and its scan_bytes BEFORE the compaction (tombstones in place);
  - the wall time of vrod_index_compact (a synchronous call: host-side plan, upload of the per-word bases, every row
    move, the tail memsets) and, in the same process, of a plain device-to-device copy of as many bytes as the
    surviving rows hold (torch, timed by events and by the wall clock) -- the yardstick;
  - the same search AFTER the compaction.
Then the update: 1 % and 10 % of the rows at random ids, wall time of vrod_index_update against vrod_index_add of the
same number of rows on the same handle (both are bound by the host-to-device upload).
Prints one JSON line per measurement.

    python scripts/probes/compact_probe.py [--rows 10000000] [--batches 10] [--warmup 3]
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
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-update", action="store_true")
    a = ap.parse_args()
    print(json.dumps({"probe": "compact", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    oi = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev)
    os_ = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(7)

    def search_ms(ix):
        wall = []
        for b in range(a.warmup + a.batches):
            torch.cuda.synchronize()
            t = time.perf_counter()
            ix.search_synthetic_device(QUERY_SEED, (b % 8) * a.nq, a.nq, a.k, oi, os_)
            torch.cuda.synchronize()
            if b >= a.warmup:
                wall.append((time.perf_counter() - t) * 1e3)
        st = ix.last_stats()
        return {"wall_ms_median": round(float(np.median(wall)), 4), "wall_ms_min": round(float(np.min(wall)), 4),
                "scan_bytes": st["scan_bytes"], "scan_launches": st["scan_launches"], "fallback_queries": st["fallback_queries"]}

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ev, wall = [], []
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t) * 1e3)
            ev.append(e0.elapsed_time(e1))
        del src, dst
        torch.cuda.empty_cache()
        return round(min(ev[1:]), 4), round(min(wall[1:]), 4)

    patterns = {"random10": lambda n: rng.choice(n, n // 10, replace=False), "random50": lambda n: rng.choice(n, n // 2, replace=False),
                "prefix30": lambda n: np.arange(n * 3 // 10)}
    for name, pick in patterns.items():
        with va.Index(a.dim, "bf16", "cosine") as ix:
            ix.reserve(a.rows)
            ix.add_synthetic(CORPUS_SEED, 0, a.rows)
            ix.delete(pick(a.rows))
            live = ix.live_count()
            before = search_ms(ix)
            torch.cuda.synchronize()
            t = time.perf_counter()
            ix.compact()
            compact_ms = (time.perf_counter() - t) * 1e3
            assert ix.count == live
            after = search_ms(ix)
        live_bytes = live * a.dim * 2
        ev_ms, wall_ms = copy_ms(live_bytes)
        print(json.dumps({"pattern": name, "live_rows": live, "live_bytes": live_bytes, "compact_wall_ms": round(compact_ms, 3),
                          "copy_event_ms": ev_ms, "copy_wall_ms": wall_ms, "ratio_to_copy_event": round(compact_ms / ev_ms, 3),
                          "search_before": before, "search_after": after}), flush=True)

    if not a.skip_update:
        with va.Index(a.dim, "bf16", "cosine") as ix:
            ix.reserve(a.rows + a.rows // 10)
            ix.add_synthetic(CORPUS_SEED, 0, a.rows)
            for frac in (0.01, 0.1):
                n = int(a.rows * frac)
                ids = rng.choice(a.rows, n, replace=False)
                rows = rng.standard_normal((n, a.dim), dtype=np.float32)
                t = time.perf_counter()
                ix.update(ids, rows)
                upd = time.perf_counter() - t
                t = time.perf_counter()
                ix.add(rows)
                add = time.perf_counter() - t
                ix.delete(np.arange(ix.count - n, ix.count))
                ix.compact()                          # a deleted suffix: nothing moves, the rows are free again
                print(json.dumps({"update_rows": n, "update_wall_s": round(upd, 4), "add_wall_s": round(add, 4),
                                  "ratio": round(upd / add, 3)}), flush=True)


if __name__ == "__main__":
    main()
