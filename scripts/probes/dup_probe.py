"""What duplicate-row detection costs: 1M x 768 cosine handles, synthetic rows, with 0 %, 5 % and 50 % of the rows made
exact copies of other rows (bf16), and once on F32 without copies.

Per handle, in one process:
  find_duplicates   wall time of the stats-only call, of the _device form (the map stays on the device) and of the host
                    form (the map crosses: 8 bytes per row);
  the hash pass     alone, from the events the library records around it under VROD_DEBUG_DUP_TIMING=1 (one JSON line on
                    stderr per call, captured here), and its effective rate: live-row bytes / time;
  the yardstick     a 1-query search through the stream scan with profiling on: scan_bytes / scan_ms of code this feature
                    does not touch, on the same handle.  ratio = hash rate / scan rate;
  the table         slots and max_probe of the call;
  delete            delete_duplicates, once, last.
The results are checked before a time is reported: duplicates must equal the copies planted.

    python scripts/probes/dup_probe.py [--rows 1000000] [--batches 7] [--warmup 2] > dup_probe_1Mx768.jsonl
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

os.environ["VROD_DEBUG_DUP_TIMING"] = "1"            # read once by the library, at the first call
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import vrod_amd as va  # noqa: E402


class Stderr:
    """The library's stderr lines of a block, parsed as JSON."""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        self.lines = []
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        for line in self.tmp.read().decode("utf-8", "replace").splitlines():
            if line.startswith('{"vrod_dup_hash_ms"'):
                self.lines.append(json.loads(line))
        self.tmp.close()


def timed(fn, warmup, batches):
    out, last = [], None
    for b in range(warmup + batches):
        torch.cuda.synchronize()
        t = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        if b >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    def emit(rec):
        print(json.dumps(rec), flush=True)
    emit({"probe": "dup", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)})
    n, dim = a.rows, a.dim
    raw = va.synth_rows_device(0, 1, 0, n, dim)
    q1 = va.synth_rows_device(0, 2, 0, 1, dim)
    for dtype, frac in (("bf16", 0.0), ("bf16", 0.05), ("bf16", 0.5), ("f32", 0.0)):
        x = raw.clone()
        copies = int(n * frac)
        if copies:                                   # the last `copies` rows (shuffled positions) become copies of earlier distinct rows
            perm = torch.randperm(n, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
            dst, src = perm[:copies], perm[copies:][torch.randint(0, n - copies, (copies,), device="cuda", generator=torch.Generator("cuda").manual_seed(8))]
            x[dst] = x[src]
        with va.Index(dim, dtype, "cosine") as ix:
            ix.reserve(n)
            ix.add_device(x)
            del x
            esize = 2 if dtype == "bf16" else 4
            row_bytes = n * dim * esize
            with Stderr() as err:
                ms_stats, min_stats, st = timed(lambda: stats_only(ix), a.warmup, a.batches)
            assert st["duplicates"] == copies and st["live"] == n, st
            hash_ms = float(np.median([l["vrod_dup_hash_ms"] for l in err.lines[a.warmup:]]))
            buf = torch.empty(n, dtype=torch.int64, device="cuda")
            with Stderr():
                ms_dev, min_dev, _ = timed(lambda: ix.find_duplicates_device(out_first=buf), a.warmup, a.batches)
                ms_host, min_host, _ = timed(lambda: ix.find_duplicates(), a.warmup, a.batches)
            # the yardstick: the stream scan of a 1-query search on the same handle
            ix.set_path(va.PATH_STREAM)
            ix.set_profiling(1)
            rates = []
            for _ in range(a.warmup + a.batches):
                ix.search_device(q1, 10)
                torch.cuda.synchronize()
                s = ix.last_stats()
                rates.append(s["scan_bytes"] / (s["scan_ms"] * 1e-3))
            ix.set_profiling(0)
            ix.set_path(va.PATH_AUTO)
            scan_rate = float(np.median(rates[a.warmup:]))
            hash_rate = row_bytes / (hash_ms * 1e-3)
            with Stderr():
                torch.cuda.synchronize()
                t = time.perf_counter()
                died = ix.delete_duplicates()
                delete_ms = (time.perf_counter() - t) * 1e3
            assert died == copies and ix.live_count() == n - copies
            emit({"dtype": dtype, "rows": n, "dim": dim, "planted_copies": copies, "stats": st,
                  "find_stats_only_ms": {"median": ms_stats, "min": min_stats},
                  "find_device_ms": {"median": ms_dev, "min": min_dev}, "find_host_ms": {"median": ms_host, "min": min_host},
                  "hash_pass_ms": hash_ms, "live_row_bytes": row_bytes, "hash_GBps": hash_rate / 1e9,
                  "stream_scan_GBps": scan_rate / 1e9, "stream_scan_ms": s["scan_ms"], "hash_over_scan": hash_rate / scan_rate,
                  "delete_duplicates_ms": delete_ms})


def stats_only(ix):
    import ctypes as C
    from vrod_amd._lib import DupStats, check
    st = DupStats()
    check(ix._L.vrod_index_find_duplicates(ix._h, 0, None, 0, C.byref(st)))
    return st.as_dict()


if __name__ == "__main__":
    main()
