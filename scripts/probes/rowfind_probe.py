"""What row lookup costs: a 1M x 768 bf16 cosine handle of synthetic rows; batches of 1 024 and 100 000 inputs that are
all new, all copies of stored rows, and half / half.

Per batch, in one process, on the same handle:
  find_rows         wall time of the _device form (the ids stay on the device), median of the timed calls;
  its passes        from the events the library records under VROD_DEBUG_ROWFIND_TIMING=1 (one JSON line on stderr per
                    call, captured here): the corpus hash pass (rate: live-row bytes / time) and the probe pass of each
                    lookup batch (rate: 8 bytes per corpus row / time);
  add_unique        one call (it changes the handle), its passes and the host time of its appends; then plain add_device
                    of the rows it appended, for the price of the lookup; the handle is brought back to its rows by
                    delete + compact after each;
  the yardstick     find_duplicates, stats only, on the same handle in the same run.
The results are checked before a time is reported: found / repeats / appended must be what the batch was built to give.

    python scripts/probes/rowfind_probe.py [--rows 1000000] [--batches 7] [--warmup 2] > rowfind_probe_1Mx768.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

os.environ["VROD_DEBUG_ROWFIND_TIMING"] = "1"        # read once by the library, at the first call
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
            if line.startswith('{"vrod_rowfind_hash_ms"'):
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


def once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def dup_stats_only(ix):
    from vrod_amd._lib import DupStats, check
    st = DupStats()
    check(ix._L.vrod_index_find_duplicates(ix._h, 0, None, 0, C.byref(st)))
    return st.as_dict()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inputs", type=int, nargs="+", default=[1024, 100_000])
    a = ap.parse_args()

    def emit(rec):
        print(json.dumps(rec), flush=True)
    emit({"probe": "rowfind", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)})
    n, dim = a.rows, a.dim
    raw = va.synth_rows_device(0, 1, 0, n, dim)
    row_bytes = n * dim * 2
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.reserve(n + max(a.inputs))
        ix.add_device(raw)

        def restore():
            """The handle back at its n rows: what a call appended is deleted and compacted away."""
            if ix.count > n:
                ix.delete(np.arange(n, ix.count, dtype=np.uint64))
                ix.compact()
            assert ix.count == n == ix.live_count()

        dup_ms, dup_min, dst = timed(lambda: dup_stats_only(ix), a.warmup, a.batches)
        assert dst["duplicates"] == 0 and dst["live"] == n, dst
        emit({"yardstick": "find_duplicates, stats only", "rows": n, "dim": dim, "ms": {"median": dup_ms, "min": dup_min}, "stats": dst})
        for m in a.inputs:
            new = va.synth_rows_device(0, 3, 0, m, dim)
            pick = torch.randint(0, n, (m,), device="cuda", generator=torch.Generator("cuda").manual_seed(m))
            n_distinct = int(torch.unique(pick[m // 2:]).numel()), int(torch.unique(pick).numel())
            for mix, t, want in (("all new", new, {"found": 0, "repeats": 0, "appended": m}),
                                 ("all copies", raw[pick], {"found": m, "repeats": 0, "appended": 0}),
                                 ("half / half", torch.cat([new[:m // 2], raw[pick[m // 2:]]]), {"found": m - m // 2, "repeats": 0, "appended": m // 2})):
                t = t.contiguous()
                buf = torch.empty(m, dtype=torch.int64, device="cuda")
                with Stderr() as err:
                    find_ms, find_min, (_, st) = timed(lambda: ix.find_rows_device(t, out_ids=buf), a.warmup, a.batches)
                assert st["found"] == want["found"] and st["repeats"] == 0 and st["appended"] == 0, st
                lines = err.lines[a.warmup:]
                hash_ms = float(np.median([l["vrod_rowfind_hash_ms"] for l in lines]))
                probe_ms = float(np.median([l["probe_ms"] / l["batches"] for l in lines]))
                with Stderr() as err:
                    add_ms, (_, ast) = once(lambda: ix.add_unique_device(t, out_ids=buf))
                assert {k: ast[k] for k in want} == want and ix.count == n + want["appended"], ast
                ids = buf.cpu().numpy().view(np.uint64)
                appended = t[torch.from_numpy((ids >= n).astype(np.bool_)).cuda()].contiguous()
                restore()
                plain_ms = None
                if len(appended):
                    plain_ms, _ = once(lambda: ix.add_device(appended))
                    restore()
                emit({"inputs": m, "mix": mix, "rows": n, "dim": dim, "dtype": "bf16", "distinct_copies": n_distinct, "find_stats": st, "add_stats": ast,
                      "find_rows_device_ms": {"median": find_ms, "min": find_min}, "find_over_find_duplicates": find_ms / dup_ms,
                      "hash_pass_ms": hash_ms, "hash_GBps": row_bytes / (hash_ms * 1e-3) / 1e9,
                      "probe_pass_ms_per_batch": probe_ms, "probe_bytes": n * 8, "probe_GBps": n * 8 / (probe_ms * 1e-3) / 1e9,
                      "add_unique_device_ms": add_ms, "add_unique_passes": err.lines[-1] if err.lines else None,
                      "plain_add_device_ms_of_the_appended": plain_ms})


if __name__ == "__main__":
    main()
