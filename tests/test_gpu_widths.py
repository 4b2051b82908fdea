"""Every handle operation at odd and very long row widths: one handle and the plain-Python model of a handle
(index_model.ModelIndex) driven side by side through ONE fixed script (sequence_exec.Pair), every step's state and every
search compared with the model bit for bit -- ids, score bits, NaN positions, labels, lims.

The core search is pinned at awkward widths by test_gpu_random.py and the long-row tests; what a handle learnt later
(deletion, the filter and its gather path, range search, update, compaction, labels, labelled and grouped search, search
by stored id, the k-NN graph) brought kernels of its own whose edges are widths no other module reaches:
  1, 3        fewer elements than one 16-B unit: the whole row is tail.  Cosine at width 1 scores +-1 only: massive ties,
              and the by-id self drop has to go by id
  31, 33      either side of one fp32 line; 33 has dim & 3 != 0 (the by-id gather's scalar branch) and ld = 64 for both types
  65          ld = 96 (fp32) and 128 (bf16): the two types pad differently
  129, 257    odd; 3 and 5 bf16 K tiles
  1100        a multiple of 4, not of 8: bf16's partial 16-B unit on the gather's vector branch
  4100        past the 4096 elements at which 8 stream queries fit in LDS; not a multiple of 8
  32768       VROD_MAX_DIM: the largest LDS request of the rescore, range and prepare kernels
Each width runs on an fp32 handle (VROD_F32_SPLIT=1, so that the [hi | lo] planes exist) and on a bf16 handle.  The three
metrics rotate over the widths: the two handles of a width take two of them, and the third gets a handle of one of the two
types (alternating), so that every width sees all three metrics in three runs of the script, not six.  That third run is
a case of its own: two runs in one case take 2.5 s at width 32768, longer than any case of test_gpu_sequence.py.  Widths
33, 257 and 4100 also run on an fp32 handle without planes (VROD_F32_SPLIT=0), and width 33 on a two-device bf16 handle
(the steps a composite handle supports).

Row counts are small and never a multiple of 256 (the last row tile is partial); the largest oracle call is
n * nq * dim = 600 * 64 * 32768 = 1.3e9, under the 2.5e9 cap of test_gpu_random.py.

Step 3 deletes row 0 and the last row, as it must; a deleted row can be neither updated nor searched by its id, so steps
4 and 7 take the first and the last LIVE row (rows 1 and n - 2, kept live for this, each next to a tombstone).
"""
import numpy as np
import pytest

import sequence_plans as S
from sequence_exec import Pair
from support import PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER

WIDTHS = (1, 3, 31, 33, 65, 129, 257, 1100, 4100, 32768)
ROWS = {1: 5003, 3: 4999, 31: 4001, 33: 3501, 65: 3333, 129: 3001, 257: 3003, 1100: 1500, 4100: 1500, 32768: 600}
METRICS = ("cosine", "l2", "ip")
NO_PLANES = (33, 257, 4100)
K = 10
L_SMALL, N_SMALL, SMALL_ROWS = S.L_SMALL0, 5, 20


def all_cases():
    """(width, dtype, metric, VROD_F32_SPLIT)."""
    out = []
    for i, w in enumerate(WIDTHS):
        m = [METRICS[(i + j) % 3] for j in range(3)]
        out += [(w, "f32", m[0], "1"), (w, "bf16", m[1], None)]
        out.append((w, "f32", m[2], "1") if i % 2 else (w, "bf16", m[2], None))
        if w in NO_PLANES:
            out.append((w, "f32", m[0], "0"))
    return out


CASES = all_cases()


def test_the_cases_cover_every_width_type_and_metric():
    assert all(n % 256 and n * 64 * w <= 2.5e9 for w, n in ROWS.items())
    for w in WIDTHS:
        mine = [c for c in CASES if c[0] == w and c[3] != "0"]
        assert len(mine) == 3 and {c[1] for c in mine} == {"f32", "bf16"} and {c[2] for c in mine} == set(METRICS)
    assert sorted(c[0] for c in CASES if c[3] == "0") == sorted(NO_PLANES)
    assert all(c[3] in ("0", "1") for c in CASES if c[1] == "f32") and all(c[3] is None for c in CASES if c[1] == "bf16")
    assert len(CASES) == 3 * len(WIDTHS) + len(NO_PLANES) and len(set(CASES)) == len(CASES)


@pytest.fixture(scope="module")
def va(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import vrod_amd
    vrod_amd.load()
    return vrod_amd


def op_search(p, rq):
    return S.Op("search", dict(rq=rq, k=K))


def plain_searches(p, tag):
    """Step 2: the stream route, the batched route at 9 and 40 queries, the exact route."""
    split = p.cfg.dtype == "f32" and p.cfg.split == "1"
    p.routed(op_search(p, p.queries(3)), PATH_STREAM, f"{tag}: 3 queries")
    p.routed(op_search(p, p.queries(9)), PATH_MFMA, f"{tag}: 9 queries, batched", force=PATH_MFMA)
    st = p.routed(op_search(p, p.queries(40)), PATH_MFMA, f"{tag}: 40 queries")
    assert st["split_pass"] == (1 if split else 0), (tag, st)
    p.routed(op_search(p, p.queries(9)), PATH_EXACT, f"{tag}: 9 queries, exact", force=PATH_EXACT)


def filtered_searches(p, path, force, tag):
    """Step 5 at one filter: top-k and range searches at 1, 9 and 40 queries, the range's threshold each query's 10th best
    eligible score -- the boundary is inclusive, so every query returns at least those ten."""
    assert p.model.filter_count() >= K
    for nq in (1, 9, 40):
        rq = p.queries(nq)
        p.routed(op_search(p, rq), path, f"{tag}: {nq} queries", force=force)
        thr = p.rank_thresholds(rq, K)
        assert np.isfinite(thr).all()
        if force is not None:
            p.ix.set_path(force)
        try:
            lims = p.check(S.Op("range_search", dict(rq=rq, thr=thr)), f"{tag}: range, {nq} queries")[0]
            st = p.ix.last_stats()
        finally:
            p.ix.set_path(PATH_AUTO)
        assert st["path"] == path, (tag, nq, st)
        assert (np.diff(lims.astype(np.int64)) >= K).all(), f"{tag}: a range search at the 10th best score returns fewer than ten rows"


def range_without_filter(p, tag):
    """Step 9: thresholds at the best and the 10th best score and at both infinities, on the default route and exactly."""
    rq = p.queries(8)
    thr = np.empty(8, np.float32)
    thr[0::4], thr[1::4] = p.rank_thresholds(rq, 1)[0::4], p.rank_thresholds(rq, K)[1::4]
    thr[2::4], thr[3::4] = np.inf, -np.inf
    op = S.Op("range_search", dict(rq=rq, thr=thr))
    n = p.model.live_count()
    for path, force in ((PATH_MFMA, None), (PATH_EXACT, PATH_EXACT)):
        if force is not None:
            p.ix.set_path(force)
        try:
            lims = p.check(op, f"{tag}: range, path {path}")[0]
            st = p.ix.last_stats()
        finally:
            p.ix.set_path(PATH_AUTO)
        assert st["path"] == path, (tag, st)
        got = np.diff(lims.astype(np.int64))
        everything = 3 if p.model.form == 0 else 2              # (the infinity that every score reaches: -inf for a dot product, +inf for a distance)
        assert (got[0::4] >= 1).all() and (got[1::4] >= K).all() and (got[everything::4] == n).all() and (got[5 - everything::4] == 0).all(), (tag, got)


def script(p, n, composite=False):
    rng = np.random.default_rng(p.seed)
    m, dim = p.model, p.cfg.dim
    split = p.cfg.dtype == "f32" and p.cfg.split == "1"

    # 1. add in two calls: the second outgrows the first allocation
    first = n * 3 // 5
    p.add(p.fresh_rows(first))
    cap = m.capacity
    p.add(p.fresh_rows(n - first))
    assert m.capacity > cap and m.count == n
    p.read_back([0, n // 2, n - 1], "step 1")

    # 2. plain searches on every route
    plain_searches(p, "step 2")

    # 3. a scattered tenth deleted: row 0, the last row, both sides of a mask word boundary (31 | 32, 63 | 64)
    keep = np.array([1, 30, 33, 62, 65, n - 2])                 # (live neighbours for step 4)
    pool = np.setdiff1d(np.arange(n), keep)
    dead = np.union1d(rng.choice(pool, n // 10, replace=False), [0, 31, 32, 63, 64, n - 1])
    p.delete(dead)
    plain_searches(p, "step 3")

    # 4. 50 rows updated in place: the first and the last live row, rows next to tombstones
    live = np.flatnonzero(~m.deleted)
    assert live[0] == 1 and live[-1] == n - 2
    touched = np.concatenate([keep, rng.choice(np.setdiff1d(live, keep), 50 - keep.size, replace=False)])
    new = p.fresh_rows(50)
    p.update(touched, new)
    p.read_back(np.unique(np.clip(np.concatenate([touched - 1, touched, touched + 1]), 0, n - 1)), "step 4")
    st = p.routed(op_search(p, np.concatenate([new[:20], p.queries(20)])), PATH_MFMA, "step 4: 40 queries, 20 of them the new rows")
    if split:                                                   # (a stale plane of an updated row: a fast score far from its canonical score)
        assert st["split_pass"] == 1 and st["max_fast_err"] <= st["eps_bound"], st

    # 5. the filter: narrow (the gather route by AUTO's own choice), then broad under the batched route
    live = np.flatnonzero(~m.deleted)
    narrow = np.zeros(n, bool)
    narrow[rng.choice(live, max(16, n // 50), replace=False)] = True
    narrow[dead[:3]] = True                                     # (allowed and deleted: not eligible)
    p.set_filter(narrow)
    filtered_searches(p, PATH_GATHER, None, "step 5, about 2 % allowed")
    p.set_filter(rng.random(n) < 0.6)
    filtered_searches(p, PATH_MFMA, PATH_MFMA, "step 5, 60 % allowed")
    p.set_filter(None)

    if not composite:
        # 6. labels: five of 20 rows, one on all other rows
        lab = np.full(n, S.L_BIG, np.uint32)
        perm = rng.permutation(n)
        for j in range(N_SMALL):
            lab[perm[SMALL_ROWS * j:SMALL_ROWS * (j + 1)]] = L_SMALL + j
        p.set_labels(0, lab)

        def aimed(labels):
            """A query per label, near a live row of it (a fresh vector for a label nobody has)."""
            rq = p.queries(len(labels))
            for q, L in enumerate(labels):
                rows = np.flatnonzero((m.labels == L) & ~m.deleted)
                if rows.size:
                    rq[q] = m.rows[rows[q % rows.size]] + np.float32(0.1) * rq[q]
            return rq, np.array(labels, np.uint32)

        def labelled(labels, tag):
            rq, ql = aimed(labels)
            p.check(S.Op("search_labeled", dict(rq=rq, k=K, qlabels=ql)), tag)
            return p.ix.last_stats()["path"]

        small = [L_SMALL + 1, L_SMALL + 1, L_SMALL + 3]
        assert labelled(small + [S.L_NOBODY], "step 6: small labels and the empty one") == PATH_GATHER     # the segment kernel alone
        assert labelled([S.L_BIG] * 3, "step 6: the big label") == PATH_STREAM                              # the dense route: an ordinary search
        labelled((small + [S.L_BIG, S.L_NOBODY]) * 2, "step 6: mixed")
        p.check(S.Op("search_grouped", dict(rq=p.queries(9), k=3)), "step 6")

        # 7. by stored id: a repeated id, the first and the last live row; the graph of rows 0 .. 63, tombstones among them
        live = np.flatnonzero(~m.deleted)
        for nq in (1, 9, 40):
            ids = np.concatenate([live[[0, -1, 0]], rng.choice(live, 37, replace=False)])[:nq].astype(np.uint64) + np.uint64(m.offset)
            for ex in (False, True):
                p.check(S.Op("search_by_ids", dict(ids=ids, k=K, exclude_self=ex)), f"step 7: {nq} ids")
        assert m.deleted[:64].sum() >= 4
        p.check(S.Op("knn_graph", dict(k=5, first_id=m.offset, n=64)), "step 7")

        # 8. compaction, then every route again
        p.compact()
        assert m.count == n - dead.size
        plain_searches(p, "step 8")

    # 9. range searches without a filter
    range_without_filter(p, "step 9")


@pytest.mark.gpu
def test_two_device_handle_at_width_33(va):
    cfg = S.Config("33-bf16-l2-two-devices", 33, "bf16", "l2")
    with Pair(va, cfg, 7999, devices=[0, 0]) as p:
        script(p, ROWS[33], composite=True)


@pytest.mark.gpu
@pytest.mark.parametrize("width,dtype,metric,split", CASES, ids=[f"{w}-{t}-{mt}" + ("-noplanes" if sp == "0" else "") for w, t, mt, sp in CASES])
def test_every_operation_at_this_width(va, width, dtype, metric, split):
    cfg = S.Config(f"{width}-{dtype}-{metric}-split{split}", width, dtype, metric, split=split)
    with Pair(va, cfg, 7000 + width) as p:
        script(p, ROWS[width])
