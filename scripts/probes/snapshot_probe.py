"""What saving and loading a handle costs: bf16 cosine synthetic rows (the benchmark's generator, built on the device), a
snapshot on the machine's temporary directory, wall times of the whole calls, median after a warm-up.

  save, load        vrod_index_save / vrod_index_load of the handle, with VROD_DEBUG_SNAPSHOT_TIMING=1: the library's own
                    line on stderr splits the call into the pack / unpack kernel and the copy (HIP events per chunk, summed),
                    the file I/O and the host's waits for the device (host clock).  The file is rewritten / reread from
                    the page cache after the first pass: the disk the numbers stand for is stated by `file_io`.
  rebuild           the yardstick of a load: vrod_index_add of the same rows as fp32 from host memory into a fresh handle
                    (what a restart did before snapshots: twice the bytes over the link, and the prepare kernels).
  file_io           plain write + fsync and plain read of as many bytes on the same directory: what the disk alone takes.
  checksum_kernel   vrod_snapshot_checksum_device over a resident buffer of the rows' size.
  pack_kernel       from the save's line: dense bytes read + dense bytes written per second of the pack kernel's own time.
One JSON line per measurement.

    python scripts/probes/snapshot_probe.py [--rows 1000000] [--dim 768] [--reps 3] [--dir /tmp]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import vrod_amd as va  # noqa: E402


def with_stderr_lines(fn):
    """fn() with the process's stderr (the library's, not only Python's) collected -> (fn's result, the lines)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode("utf-8", "replace").splitlines()


def timed_call(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out, lines = with_stderr_lines(fn)
    wall = (time.perf_counter() - t) * 1e3
    own = [json.loads(x) for x in lines if x.startswith('{"vrod_snapshot"')]
    return out, wall, (own[-1] if own else {})


def median_of(runs):
    walls = [w for w, _ in runs]
    mid = runs[int(np.argsort(walls)[len(walls) // 2])]
    return {"wall_ms_median": round(mid[0], 1), "wall_ms_min": round(min(walls), 1), "split_of_median": mid[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    a = ap.parse_args()
    os.environ["VROD_DEBUG_SNAPSHOT_TIMING"] = "1"
    print(json.dumps({"probe": "snapshot", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    path = os.path.join(a.dir, f"vrod_snapshot_probe_{os.getpid()}.vrod")
    dense = a.rows * a.dim * 2
    try:
        ix = va.Index(a.dim, "bf16", "cosine")
        ix.add_synthetic(1, 0, a.rows)
        q = va.synth_rows_device(0, 2, 0, 64, a.dim).cpu().numpy()
        want = ix.search(q, 10)

        runs = []
        for r in range(a.reps + 1):
            _, wall, own = timed_call(lambda: ix.save(path))
            if r:
                runs.append((wall, own))
        save = median_of(runs)
        size = os.path.getsize(path)
        print(json.dumps({"what": "save", "file_bytes": size, **save}), flush=True)
        k_ms = save["split_of_median"].get("pack_kernel_ms")
        if k_ms:
            print(json.dumps({"what": "pack_kernel", "kernel_ms": k_ms, "dense_bytes": dense,
                              "TB_per_s_read_plus_written": round(2 * dense / (k_ms * 1e-3) / 1e12, 3)}), flush=True)

        runs = []
        for r in range(a.reps + 1):
            ld, wall, own = timed_call(lambda: va.Index.load(path))
            got = ld.search(q, 10)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            ld.close()
            if r:
                runs.append((wall, own))
        print(json.dumps({"what": "load", "file_bytes": size, **median_of(runs)}), flush=True)

        # the yardstick: the same handle rebuilt from fp32 rows in host memory
        raw = np.empty((a.rows, a.dim), np.float32)
        step = 1 << 17
        for r0 in range(0, a.rows, step):
            raw[r0:r0 + step] = va.synth_rows_device(0, 1, r0, min(step, a.rows - r0), a.dim).cpu().numpy()
        walls = []
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fresh = va.Index(a.dim, "bf16", "cosine")
            fresh.add(raw)
            wall = (time.perf_counter() - t) * 1e3
            got = fresh.search(q, 10)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            fresh.close()
            if r:
                walls.append(wall)
        print(json.dumps({"what": "rebuild", "fp32_bytes": raw.nbytes, "wall_ms_median": round(float(np.median(walls)), 1),
                          "wall_ms_min": round(min(walls), 1)}), flush=True)

        # the disk alone
        blob = raw.view(np.uint8).reshape(-1)[:size]
        wr, rd = [], []
        for r in range(a.reps):
            t = time.perf_counter()
            with open(path + ".plain", "wb") as f:
                f.write(blob)
                f.flush()
                os.fsync(f.fileno())
            wr.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            with open(path + ".plain", "rb") as f:
                f.readinto(memoryview(blob))
            rd.append((time.perf_counter() - t) * 1e3)
        print(json.dumps({"what": "file_io", "bytes": size, "write_fsync_ms_median": round(float(np.median(wr)), 1),
                          "read_ms_median": round(float(np.median(rd)), 1), "dir": a.dir}), flush=True)

        # the plain checksum kernel over resident bytes
        buf = torch.randint(0, 2 ** 31 - 1, (dense // 4,), dtype=torch.int32, device="cuda")
        L, out = va.load(), C.c_uint64()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        walls = []
        for r in range(a.reps + 2):
            torch.cuda.synchronize()
            t = time.perf_counter()
            assert L.vrod_snapshot_checksum_device(0, C.c_void_p(buf.data_ptr()), dense, 0, C.byref(out), stream) == 0
            if r >= 2:
                walls.append((time.perf_counter() - t) * 1e3)
        ms = float(np.median(walls))
        print(json.dumps({"what": "checksum_kernel", "bytes": dense, "call_ms_median": round(ms, 3),
                          "TB_per_s": round(dense / (ms * 1e-3) / 1e12, 3)}), flush=True)
        ix.close()
    finally:
        for p in (path, path + ".tmp", path + ".plain"):
            if os.path.exists(p):
                os.remove(p)


if __name__ == "__main__":
    main()
