"""What row keys cost: a bf16 cosine handle of synthetic rows (the benchmark's generator, built on the device) with every
row keyed, then the four numbers profiles/keys/README.md records.

  add, set_keys     vrod_index_add_synthetic of all rows, then ONE vrod_index_set_keys over all of them (keys in host
                    memory: the host's duplicate check, the copy of the column, the table built by the rebuild kernel).
  find              vrod_index_find_keys_device on --find keys in device memory, half held and half unknown: keys per
                    second, and the average walk in slots from the library's own line (VROD_DEBUG_KEYS_WALK=1).
  translate         vrod_index_ids_to_keys_device on a 1024 x 10 id list in device memory.
  upsert            vrod_index_upsert of --upsert rows from host memory, half of them new, against the same work through
                    vrod_index_update + vrod_index_add + vrod_index_set_keys on the same handle.
Clocks: the host's perf_counter around whole calls; every call timed here is synchronous and returns after a stream
synchronise.  Each shape runs once untimed first; then the median of --reps runs (the mutating calls: one run each, on a
fresh batch).  One JSON line per measurement in <out>/keys_probe_<rows>x<dim>.jsonl, the table in <out>/README.md.

    python scripts/probes/keys_probe.py [--rows 10000000] [--dim 768] [--find 1000000] [--upsert 10000] [--reps 5] [--out profiles/keys]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--find", type=int, default=1_000_000)
    ap.add_argument("--upsert", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keys"))
    a = ap.parse_args()
    os.environ["VROD_DEBUG_KEYS_WALK"] = "1"          # read once by the library, at its first find
    import torch
    import vrod_amd as va

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t) * 1e3

    def median(fn, reps):
        fn()
        return float(np.median([wall(fn)[1] for _ in range(reps)]))

    os.makedirs(a.out, exist_ok=True)
    lines = []

    def record(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    n, dim = a.rows, a.dim
    rng = np.random.default_rng(1)
    # distinct 64-bit keys with no structure the hash could like: an odd multiplier is a bijection mod 2^64
    with np.errstate(over="ignore"):
        keys = (np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * np.uint64(0xD1342543DE82EF95)      # odd
        unknown = np.arange(1, a.find // 2 + 1, dtype=np.uint64) * np.uint64(2) * np.uint64(0xD1342543DE82EF95)    # even
    with va.Index(dim, "bf16", "cosine") as ix:
        _, add_ms = wall(lambda: ix.add_synthetic(7, 0, n))
        _, key_ms = wall(lambda: ix.set_keys(0, keys))
        st = ix.key_stats()
        record(what="add_synthetic", rows=n, dim=dim, wall_ms=round(add_ms, 1))
        record(what="set_keys", rows=n, wall_ms=round(key_ms, 1), **st)
        t = time.perf_counter()
        np.sort(keys)
        record(what="host_sort_of_the_keys_numpy", rows=n, wall_ms=round((time.perf_counter() - t) * 1e3, 1),
               note="a yardstick for the duplicate check's std::sort inside set_keys, not a split of the call")

        ask = np.concatenate([keys[rng.choice(n, a.find - unknown.size, replace=False)], unknown])
        rng.shuffle(ask)
        d_ask = torch.from_numpy(ask.view(np.int64)).cuda()
        d_out = torch.empty_like(d_ask)
        ix.find_keys_device(d_ask, out_ids=d_out)
        (_, find_ms), err = with_stderr_lines(lambda: wall(lambda: ix.find_keys_device(d_ask, out_ids=d_out)))
        own = [json.loads(x) for x in err if x.startswith('{"vrod_keys_find"')]
        find_med = median(lambda: ix.find_keys_device(d_ask, out_ids=d_out), a.reps)
        found = int((d_out.cpu().numpy().view(np.uint64) != np.uint64(0xFFFFFFFFFFFFFFFF)).sum())
        record(what="find_keys_device", keys=int(ask.size), found=found, wall_ms_median=round(find_med, 3),
               keys_per_s=round(ask.size / (find_med * 1e-3)), avg_walk_slots=round(own[-1]["slots_visited"] / ask.size, 3) if own else None,
               slots=st["slots"], occupied=st["occupied"])

        d_ids = torch.from_numpy(rng.integers(0, n, (1024, 10)).astype(np.int64)).cuda()
        d_keys = torch.empty_like(d_ids)
        tr_med = median(lambda: ix.ids_to_keys_device(d_ids, out_keys=d_keys), 4 * a.reps)
        assert np.array_equal(d_keys.cpu().numpy().view(np.uint64), keys[d_ids.cpu().numpy()])
        record(what="ids_to_keys_device", ids=int(d_ids.numel()), wall_ms_median=round(tr_med, 4))

        m = a.upsert
        half = m // 2

        def batch(b):
            """Batch b: half held keys (rows of their own), half keys no row holds yet, and the vectors."""
            held = np.arange(b * half, (b + 1) * half)
            with np.errstate(over="ignore"):
                new = (np.arange(1, m - half + 1, dtype=np.uint64) + np.uint64((b + 1) << 40)) * np.uint64(2) * np.uint64(0xD1342543DE82EF95)
            vec = np.random.default_rng(100 + b).standard_normal((m, dim)).astype(np.float32)
            return held, new, vec

        ready = []                                            # built ahead: only the library's calls are timed
        for b_ in range(6):
            held, new, vec = batch(b_)
            k = np.empty(m, np.uint64)
            k[0::2], k[1::2] = keys[held], new                # interleaved: the call splits them
            ready.append((k, vec, held.astype(np.uint64), np.ascontiguousarray(vec[0::2]), np.ascontiguousarray(vec[1::2]), new))

        def by_upsert(b):
            return ix.upsert(ready[b][0], ready[b][1])

        def by_parts(b):
            _, _, ids, vec_held, vec_new, new = ready[b]
            ix.update(ids, vec_held)
            first = ix.count
            ix.add(vec_new)
            ix.set_keys(first, new)

        by_upsert(0), by_parts(1)                             # untimed: both flows once
        _, up_ms = wall(lambda: by_upsert(2))
        _, parts_ms = wall(lambda: by_parts(3))
        _, up2_ms = wall(lambda: by_upsert(4))
        _, parts2_ms = wall(lambda: by_parts(5))
        record(what="upsert", rows=m, new=m - half, wall_ms=[round(up_ms, 2), round(up2_ms, 2)])
        record(what="update_add_set_keys", rows=m, new=m - half, wall_ms=[round(parts_ms, 2), round(parts2_ms, 2)])
        record(what="key_stats_at_the_end", **ix.key_stats())

    with open(os.path.join(a.out, f"keys_probe_{n // 1_000_000}Mx{dim}.jsonl"), "w") as f:
        f.writelines(json.dumps(x) + "\n" for x in lines)
    by = {x["what"]: x for x in lines}
    slower = key_ms > add_ms
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write(f"""# Row keys: what they cost

Written by `scripts/probes/keys_probe.py` ({va.version()}); {n} x {dim} bf16 cosine synthetic rows on one MI355X, every
row keyed.  Clocks: the host's `perf_counter` around whole synchronous calls (each returns after a stream synchronise);
every shape ran once untimed first; medians of {a.reps} runs where a call can be repeated, single runs (two batches)
for the calls that change the handle.  The raw lines are in `keys_probe_{n // 1_000_000}Mx{dim}.jsonl`.  None of these
numbers has a target; the structural condition is the table's: occupied <= slots / 2 and walks bounded by the slot count.

| measurement | result |
|---|---|
| adding the rows (`vrod_index_add_synthetic`) | {by['add_synthetic']['wall_ms']} ms |
| keying all of them, one `vrod_index_set_keys` | {by['set_keys']['wall_ms']} ms; {st['slots']} slots, {st['occupied']} occupied, longest walk {st['max_probe']} |
| numpy sort of the same keys on the host (yardstick) | {by['host_sort_of_the_keys_numpy']['wall_ms']} ms |
| `vrod_index_find_keys_device`, {by['find_keys_device']['keys']} keys, half held | {by['find_keys_device']['wall_ms_median']} ms = {by['find_keys_device']['keys_per_s']} keys/s, average walk {by['find_keys_device']['avg_walk_slots']} slots |
| `vrod_index_ids_to_keys_device`, 1024 x 10 ids | {by['ids_to_keys_device']['wall_ms_median']} ms |
| `vrod_index_upsert`, {m} rows, half new | {by['upsert']['wall_ms']} ms |
| the same rows through `update` + `add` + `set_keys` | {by['update_add_set_keys']['wall_ms']} ms |

Keying the rows took {'LONGER' if slower else 'no longer'} than adding them did ({key_ms:.0f} ms against {add_ms:.0f} ms).
{'The rows here are generated on the device, so the add moves no bytes from the host; the keying call does its work on the host first: it walks the range against the tombstone mirror, sorts the keys of the live rows to find a repeat (the yardstick above is that sort in numpy), fills and copies the host mirror, and copies 8 bytes per row to the device from pageable memory, before one rebuild launch builds the table.  The split of the call was not measured.' if slower else ''}
The call times of find and translate include the launch, the read-back of the table's counters and a stream synchronise.
An upsert does more than its parts: it sorts the call's keys to refuse a repeat, makes a prepare-only pass over every
vector before the first row is written (a second upload of the batch), looks the keys up, and splits the batch on the
host into its held and its new half (a copy of the vectors); update + add + set_keys above were handed their halves
ready-made and check nothing across the batch.  Which of these steps carries the difference was not measured.
""")


if __name__ == "__main__":
    main()
