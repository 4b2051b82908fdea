"""Leak probe: handles are created, used and destroyed 120 times; the free device memory is printed at three iterations
and must not drift downward.  Every handle runs the plain search and each of the derived searches (host forms: nothing
here allocates device memory but the library), so every workspace of the handle is grown before it is destroyed.  The
last line is the device footprint of one handle after all of them have run once.  Run from the repository root."""
import sys
sys.path.insert(0, ".")
import numpy as np, torch
import vrod_amd as va
rng = np.random.default_rng(1)
raw = rng.standard_normal((20000, 128)).astype(np.float32)
rq = rng.standard_normal((40, 128)).astype(np.float32)
labels = rng.integers(0, 500, 20000).astype(np.uint32)
tags = rng.integers(0, 64, 20000).astype(np.uint64)
some = rng.choice(20000, 80, replace=False).astype(np.uint64)
cand = rng.integers(0, 20000, 40 * 100).astype(np.uint64)
cand_lims = (np.arange(41) * 100).astype(np.uint32)


def free_mib():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0] / 2**20


def derived(ix):
    ix.set_labels(0, labels)
    ix.set_tags(0, tags)
    ix.search_labeled(rq, 10, labels[:40])
    ix.search_tagged(rq, 10, np.tile(np.array([[3, 0, 4]], np.uint64), (40, 1)))
    ix.search_grouped(rq, 10)
    ix.search_multivec(rq, 10, np.arange(0, 41, 4))
    ix.search_diverse(rq, 10, 40, 0.5)
    ix.search_by_ids(some[:40], 10, exclude_self=True)
    ix.search_combined(10, some, np.ones(80, np.float32), np.arange(0, 81, 2), rq, None, some[:40], np.arange(41), exclude_terms=True)
    ix.search_candidates(rq, 10, cand, cand_lims)
    ix.score_candidates(rq, cand, cand_lims)
    ix.knn_graph(10, 0, 2500)


for it in range(120):
    with va.Index(128, ["f32", "bf16"][it % 2], ["cosine", "l2"][(it // 2) % 2]) as ix:
        ix.add(raw)
        ix.search(rq, 10)
        ix.search(rq[:2], 10)
        derived(ix)
        if it % 3 == 0:
            with va.Index(128, "f32", "cosine", devices=[0, 0]) as mx:
                mx.add(raw); mx.search(rq[:3], 5)
    if it in (10, 60, 119):
        print(f"iteration {it}: free {free_mib():.0f} MiB")

before = free_mib()
with va.Index(128, "bf16", "cosine") as ix:
    ix.add(raw)
    base = free_mib()
    derived(ix)
    after = free_mib()
    print(f"footprint: corpus {before - base:.1f} MiB, after the derived searches {before - after:.1f} MiB")
