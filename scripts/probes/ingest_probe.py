"""What it costs to get rows that are in GPU memory into a handle: vrod_index_add from host memory (what a caller with an
encoder's output on the GPU had to do, less the cast and the copy to the host, which are not timed) against
vrod_index_add_device from an fp32, a bf16 and an fp16 tensor, on a bf16 cosine handle and on an fp32 L2 handle, in one
process; then vrod_index_update against vrod_index_update_device on --update rows, and vrod_index_add_synthetic of
--rows rows.  --host-only leaves the device sources out: the host forms alone, for a comparison of two builds of the
library (VROD_HIP_LIB names the one to load).

Clocks: the host's perf_counter around whole calls; every call timed here is synchronous and returns after a stream
synchronise.  Each handle is reserved for its rows first (no growth inside the timed call), each shape runs once untimed
on a small handle, then the median of --reps runs, each on a fresh handle.  "GB/s" is the source's bytes (rows x dim x
element size) over the call's time.  One JSON line per measurement in <out>/ingest_probe_<rows>x<dim>.jsonl.

    python scripts/probes/ingest_probe.py [--rows 1000000] [--dim 768] [--update 65536] [--reps 3] [--host-only] [--out profiles/ingest]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--update", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest"))
    a = ap.parse_args()
    import torch
    import vrod_amd as va

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    n, dim, m = a.rows, a.dim, a.update
    torch.manual_seed(1)
    src = {"f32": torch.randn((n, dim), device="cuda")}
    if not a.host_only:
        src["bf16"] = src["f32"].to(torch.bfloat16)
        src["f16"] = src["f32"].to(torch.float16)
    whats = ("host",) + (() if a.host_only else tuple(src))
    host = src["f32"].cpu().numpy()
    ids = torch.randperm(n, device="cuda")[:m].contiguous()
    host_ids = ids.cpu().numpy()
    label = f"{n // 1_000_000}M" if n % 1_000_000 == 0 else str(n)
    os.makedirs(a.out, exist_ok=True)
    lines = []

    def record(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for dtype, metric in (("bf16", "cosine"), ("f32", "l2")):
        def fresh(rows=n):
            ix = va.Index(dim, dtype, metric)
            ix.reserve(rows)
            return ix

        with fresh(4096) as ix:                                # untimed: every kernel of the timed calls has run once
            ix.add(host[:4096])
            for t in src.values():
                ix.add_device(t[:4096])
            ix.update(host_ids[:64] % 4096, host[:64])
            ix.update_device(ids[:64] % 4096, src["f32"][:64])
            ix.add_synthetic(1, 0, 4096)
        add_host = None
        for what in whats:
            times = []
            for _ in range(a.reps):
                with fresh() as ix:
                    times.append(wall((lambda: ix.add(host)) if what == "host" else (lambda: ix.add_device(src[what]))))
                    assert ix.count == n
            s = statistics.median(times)
            gb = n * dim * (4 if what in ("host", "f32") else 2) / 1e9
            add_host = s if what == "host" else add_host
            record(op="add" if what == "host" else "add_device", handle=f"{dtype}/{metric}", source=what, rows=n, dim=dim, seconds=s,
                   source_GBps=gb / s, vs_host_add=add_host / s, runs=times)
        with fresh() as ix:
            ix.add_device(src["f32"])
            for what in whats:
                times = [wall((lambda: ix.update(host_ids, host[:m])) if what == "host" else (lambda: ix.update_device(ids, src[what][:m])))
                         for _ in range(a.reps)]
                s = statistics.median(times)
                record(op="update" if what == "host" else "update_device", handle=f"{dtype}/{metric}", source=what, rows=m, dim=dim,
                       seconds=s, source_GBps=m * dim * (4 if what in ("host", "f32") else 2) / 1e9 / s, runs=times)
        times = []
        for _ in range(a.reps):
            with fresh() as ix:
                times.append(wall(lambda: ix.add_synthetic(1, 0, n)))
        record(op="add_synthetic", handle=f"{dtype}/{metric}", source="synthetic", rows=n, dim=dim, seconds=statistics.median(times), runs=times)
    with open(os.path.join(a.out, f"ingest_probe_{label}x{dim}{'_host' if a.host_only else ''}.jsonl"), "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")
    ok = all(x["seconds"] <= y["seconds"] for x in lines if x["op"] == "add_device" and x["source"] == "f32"
             for y in lines if y["op"] == "add" and y["handle"] == x["handle"])
    print("the one condition (add_device from fp32 takes no longer than add):", "holds" if ok else "FAILS")


if __name__ == "__main__":
    main()
