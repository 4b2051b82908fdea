"""What a multi-vector search costs: bf16 cosine rows of a topical synthetic corpus (topic centroids x 12 documents x 1 to
5 rows, each row its centroid plus 0.6 N(0, I) / sqrt(dim), built on the device in chunks and uploaded once), 64 queries
of 32 vectors drawn the same way around one topic each, k = 10.

Three times (median wall time of the _device form, pointers resident):
  multivec        the call on the default path (candidate route, dense for the queries it does not certify);
  multivec_exact  the same call under PATH_EXACT: the dense route for every query;
  search_at_k1    a plain vrod_search_device of the same 2048 vectors at k1: the floor the candidate route stands on.
With them the route counters of vrod_index_last_multivec (certified share, candidate labels and rows).  One JSON line per
measurement.

    python scripts/probes/multivec_probe.py [--rows 1000000] [--batches 5] [--warmup 1]
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

DOCS_PER_TOPIC, NOISE = 12, 0.6


def timed(fn, warmup, batches):
    out = []
    for b in range(warmup + batches):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(b)
        torch.cuda.synchronize()
        if b >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--vectors", type=int, default=32)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--exact-batches", type=int, default=2)
    a = ap.parse_args()
    print(json.dumps({"probe": "multivec", "box": {"device": torch.cuda.get_device_name(0), "library": va.version()}, "args": vars(a)}), flush=True)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.default_rng(1)
    # documents: 1 .. 5 rows each, DOCS_PER_TOPIC per topic, until the rows are used up
    sizes = rng.integers(1, 6, a.rows)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), a.rows)) + 1]
    doc_of_row = np.repeat(np.arange(sizes.size), sizes)[:a.rows]
    n_topics = int(doc_of_row[-1]) // DOCS_PER_TOPIC + 1
    cent = torch.nn.functional.normalize(torch.randn((n_topics, a.dim), generator=g, device=dev), dim=1)
    topic_of_row = torch.from_numpy(doc_of_row // DOCS_PER_TOPIC).to(dev)
    ix = va.Index(a.dim, "bf16", "cosine")
    ix.reserve(a.rows)
    t0 = time.perf_counter()
    for r0 in range(0, a.rows, 100_000):
        r1 = min(a.rows, r0 + 100_000)
        rows = cent[topic_of_row[r0:r1]] + NOISE * torch.randn((r1 - r0, a.dim), generator=g, device=dev) / a.dim ** 0.5
        ix.add(rows.cpu().numpy())
    ix.set_labels(0, (doc_of_row + 1).astype(np.uint32))
    print(json.dumps({"what": "corpus", "rows": a.rows, "documents": int(doc_of_row[-1]) + 1, "topics": n_topics,
                      "build_s": round(time.perf_counter() - t0, 2)}), flush=True)
    nv = a.queries * a.vectors
    qt = torch.randint(0, n_topics, (a.queries,), generator=g, device=dev).repeat_interleave(a.vectors)
    dv = (cent[qt] + NOISE * torch.randn((nv, a.dim), generator=g, device=dev) / a.dim ** 0.5).contiguous()
    dl = torch.arange(0, nv + 1, a.vectors, dtype=torch.int32, device=dev)
    ol = torch.empty((a.queries, a.k), dtype=torch.int32, device=dev)
    os_ = torch.empty((a.queries, a.k), dtype=torch.float32, device=dev)
    of = torch.empty((a.queries,), dtype=torch.int32, device=dev)

    def report(what, med, mn):
        st, mv = ix.last_stats(), ix.last_multivec()
        print(json.dumps({"what": what, "queries": a.queries, "vectors": a.vectors, "k": a.k, "wall_ms_median": round(med, 3),
                          "wall_ms_min": round(mn, 3), "path": st["path"], "fallback_queries": st["fallback_queries"],
                          "scan_launches": st["scan_launches"], "scan_bytes": st["scan_bytes"], **{"mv_" + n: v for n, v in mv.items()}}),
              flush=True)

    med, mn = timed(lambda b: ix.search_multivec_device(dv, dl, a.k, ol, os_, of), a.warmup, a.batches)
    report("multivec", med, mn)
    first = ol.clone(), os_.clone()
    k1 = ix.last_multivec()["k1"]
    pi = torch.empty((nv, k1), dtype=torch.int64, device=dev)
    ps = torch.empty((nv, k1), dtype=torch.float32, device=dev)
    med, mn = timed(lambda b: ix.search_device(dv, k1, pi, ps), a.warmup, a.batches)
    st = ix.last_stats()
    print(json.dumps({"what": "search_at_k1", "nq": nv, "k": k1, "wall_ms_median": round(med, 3), "wall_ms_min": round(mn, 3),
                      "path": st["path"], "fallback_queries": st["fallback_queries"]}), flush=True)
    ix.set_path(va.PATH_EXACT)
    med, mn = timed(lambda b: ix.search_multivec_device(dv, dl, a.k, ol, os_, of), 0, a.exact_batches)
    report("multivec_exact", med, mn)
    same = bool(torch.equal(first[0], ol) and torch.equal(first[1].view(torch.int32), os_.view(torch.int32)))
    print(json.dumps({"what": "routes_agree", "same_bits": same}), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
