"""Every search form that reaches the 4-wave scan (kernels_mfma_w4.hip), at widths whose launches take its tile loop.

launch_mfma_w4 runs a bf16 launch whose K extent is an even number of 128-byte K-tiles, at least 4, through TLOOP: a loop
over tiles around a fixed-trip K loop, with its own copies of the staging cursor's tile crossing, the work-stealing claim,
the pacing countdown and the `tile = st_tile` hand-over that gives the filter epilogue its row numbers.
tests/test_gpu_w4_tile_loop.py pins plain top-k under that loop; the row mask (tombstones, allow list), range search and
its spills, ip handles, the id offset, by-id batches, the graph, labelled and grouped searches, updates, compaction,
pipelined chains, batches of more query blocks than work-group slots and pacing points are pinned elsewhere at one to
three K-tiles only, i.e. under the flat loop.  Here they run at

    dim 256 (4 K-tiles: the pair loop runs zero times)   dim 384 (6: once)   dim 768 (12: four times)
    dim 200 (pads to 256 elements: 4 K-tiles, 56 zero columns)
    dim 192 (3) and dim 320 (5): the flat loop, on its `tile = st_tile` arm -- the controls that make a failure
    attributable to one loop form

always on a bf16 handle with PATH_MFMA forced and asserted, and with more than 64 queries (300 = two query blocks, the
second partial), so that the 4-wave kernel and not the skinny kernel takes the batch.  Every comparison is bit for bit --
ids, score bits, NaN positions, lims -- against the model (index_model.ModelIndex) or the CPU oracle.  Parity is against
this repository's own oracle: the reference project holds no scan.

A  One handle script per width against the model (sequence_exec.Pair), cut into five cases per width; a case replays the
   mutations of the cases before it (without their searches) and then runs its own steps, so any case runs alone.
   5003 rows (2003 at dim 768) fit one hit list (8192 entries), and such a corpus is scanned by ONE filtered launch
   without a sample and without a threshold: every eligible row of every query goes through the filter epilogue, the
   hit logs and the spill regions with its row number.  The staged form -- a sample launch and two filtered launches
   -- starts above 8192 rows: the last case grows its handle to 9003 rows and searches again, under the allow list.
B  60 000 rows x 300 queries at dim 256 and 384 -- static tile ranges of exactly one and exactly two tiles and a partial
   last tile -- under tombstones and an allow list, and under range search with lists redone in pieces; and a batch of 33
   query blocks (two kernel launches, the second with qb_base = 32).
C  Pacing points inside the tile loop: VROD_DEBUG_PACE_KT unset, 0 and 8 in child processes give the same bits.
tests/test_w4_forms_shapes.py checks on the CPU that these shapes still meet the conditions they were chosen for.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sequence_plans as S
from sequence_exec import Pair, same_lists
from support import (DT, PATH_AUTO, PATH_EXACT, PATH_MFMA, THREADS, assert_same_all_bits, eligible_rows, form_of, hard_thresholds,
                     oracle_over, prep_of, row_bytes, takes_segments)
from test_gpu_steal import stage_plan
from test_gpu_w4_tile_loop import sample_is_grouped, stage_strip_lens, takes_tile_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, K = 300, 10
LIST_CAP = 8192                      # entries of a query's hit list (kSelectChunk)
METRICS = ("cosine", "l2", "ip")

# dim: (K-tiles, tile loop?, metric, id offset, rows).  The metrics rotate so that each meets the tile loop.
WIDTHS = {
    256: (4, True, "cosine", 0, 5003),
    384: (6, True, "l2", 10 ** 9, 5003),
    768: (12, True, "ip", 0, 2003),
    200: (4, True, "l2", 0, 5003),
    192: (3, False, "ip", 0, 5003),
    320: (5, False, "cosine", 0, 5003),
}
PHASES = ("plain", "deleted", "byid", "filtered", "rewritten")
GROWN_ROWS = 9003                    # the last case's handle after its final add: more rows than a hit list holds
ALLOWED_SHARE = 0.6
L_BIG, L_SMALL, N_SMALL, SMALL_ROWS = S.L_BIG, S.L_SMALL0, 4, 20
B_N, B_DIMS = 60_000, (256, 384)
B_MANY_NQ, B_MANY_ROWS = 8448, 2003
C_N, C_DIMS, C_SETTINGS = 170_000, (256, 384), (None, "0", "8")


# ---------------------------------------------------------------- restated from the library (checked on the CPU too)
def k_tiles(dim):
    return row_bytes("bf16", dim) // 128


def plan_metric(metric):
    """The stage plan knows two score forms: ip takes the dot form's candidate margin (search_plan.h choose_kp)."""
    return "l2" if metric == "l2" else "cosine"


def tloop_pace_tiles(kt, pace_every, ntiles):
    """The pacing countdown of the TLOOP branch, restated: it starts at pace_every + KT, drops by KT in front of every
    tile and fires at or below zero, where it gains pace_every (pace_every = 0: never).  -> the 1-based tiles of a
    work-group's `ntiles` in front of which a pacing point stands."""
    if not pace_every:
        return []
    left, out = pace_every + kt, []
    for t in range(1, ntiles + 1):
        left -= kt
        if left <= 0:
            left += pace_every
            out.append(t)
    return out


def scan_launches(n, nq, k, metric, num_cus):
    """Scan launches of a bf16 batch (vrod_index.hip): a corpus that fits one hit list takes a single filtered launch;
    a larger one the sample launch and a filtered launch per stage bound."""
    return 1 if n <= LIST_CAP else 1 + len(stage_plan(n, nq, k, plan_metric(metric), num_cus)[2])


def deleted_stretch(n):
    """Step A2 without the queries' best rows: row 0, the last row, one whole row tile, every third row of the next."""
    return np.unique(np.concatenate([[0, n - 1], np.arange(256, 512), np.arange(512, 768, 3)]))


def allow_list(dim, n):
    """Step A7's dense allow list: about 60 % of the rows."""
    return np.random.default_rng(7000 + dim).random(n) < ALLOWED_SHARE


def worse(metric):
    """The threshold every finite score reaches."""
    return np.float32(np.inf if metric == "l2" else -np.inf)


# ---------------------------------------------------------------- fixtures
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def va(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import vrod_amd
    vrod_amd.load()
    return vrod_amd


def _cus():
    import torch
    assert torch.cuda.is_available()
    return torch.cuda.get_device_properties(0).multi_processor_count


# ================================================================ A: one handle script against the model, per width
def queries(p, phase, nq):
    """Queries of one phase, from a generator of their own: the rows' generator (p.gen) then sees the same calls in
    every case, so a case that replays the earlier mutations rebuilds the same handle."""
    return S._Maker(9000 + 16 * p.cfg.dim + phase, p.cfg, p.model).queries(nq)


def search(p, rq, k, tag):
    st = p.routed(S.Op("search", dict(rq=rq, k=k)), PATH_MFMA, tag)
    assert st["nq"] == rq.shape[0] and st["k"] == k, (tag, st)
    return st


def range_search(p, rq, thr, tag):
    lims = p.check(S.Op("range_search", dict(rq=rq, thr=thr)), tag)[0]
    st = p.ix.last_stats()
    assert st["path"] == PATH_MFMA, (tag, st)
    return np.diff(lims.astype(np.int64)), st


def build(p, n):
    """The handle of every case: n rows in two calls (the second outgrows the first allocation), the path forced."""
    first = n * 3 // 5
    p.add(p.fresh_rows(first))
    cap = p.model.capacity
    p.add(p.fresh_rows(n - first))
    assert p.model.capacity > cap and p.model.count == n and n % 256 != 0
    p.set_path(PATH_MFMA)


def delete(p, n):
    """Step 2's mutation -> (the step's 300 queries, the best rows their first 100 had)."""
    m = p.model
    rq = queries(p, 2, NQ)
    best = (m.search(rq[:100], 1)[0][:, 0] - np.uint64(m.offset)).astype(np.int64)
    dead = np.union1d(deleted_stretch(n), best)
    p.delete(dead)
    # from the model alone: each of the 100 queries has lost its best row, whichever tile it stood in
    now = (m.search(rq[:100], 1)[0][:, 0] - np.uint64(m.offset)).astype(np.int64)
    assert m.deleted[best].all() and not m.deleted[now].any() and (now != best).all()
    return rq, best


def set_allow_list(p, n):
    allow = allow_list(p.cfg.dim, n)
    p.set_filter(allow)
    m, dim = p.model, p.cfg.dim
    elig = m.filter_count()
    assert 0.4 * n < elig < 0.65 * n
    # a dense list: AUTO itself would scan under the mask and not gather, and so does the forced path
    assert not takes_segments(PATH_AUTO, "bf16", n, elig, NQ, dim) and not takes_segments(PATH_MFMA, "bf16", n, elig, NQ, dim)


def set_label_plan(p, n):
    """One label on ~60 % of the rows, N_SMALL labels of SMALL_ROWS rows, label 0 on the rest."""
    rng = np.random.default_rng(7100 + p.cfg.dim)
    lab = np.zeros(n, np.uint32)
    perm = rng.permutation(n)
    lab[perm[:n * 3 // 5]] = L_BIG
    for j in range(N_SMALL):
        lab[perm[n * 3 // 5 + SMALL_ROWS * j:n * 3 // 5 + SMALL_ROWS * (j + 1)]] = L_SMALL + j
    p.set_labels(0, lab)


def phase_plain(p, n):
    """Step 1 on the fresh handle: 300 queries, 257 (one live query in the second block), k = 100."""
    st = search(p, queries(p, 1, NQ), K, "step 1: 300 queries")
    assert n <= LIST_CAP and st["scan_launches"] == scan_launches(n, NQ, K, p.cfg.metric, _cus()) == 1, st   # one filtered launch over every row
    search(p, queries(p, 11, 257), K, "step 1: 257 queries")
    search(p, queries(p, 12, NQ), 100, "step 1: k = 100")


def phase_deleted(p, n):
    """Steps 2 - 4: tombstones in the filter epilogue, range search, a range search whose every tile spills."""
    m = p.model
    rq, _ = delete(p, n)
    search(p, rq, K, "step 2: after the delete")
    rq = queries(p, 3, NQ)
    thr = p.rank_thresholds(rq, K)
    assert np.isfinite(thr).all()
    counts, _ = range_search(p, rq, thr, "step 3: range at the 10th best score")
    assert (counts >= K).all(), counts[counts < K]
    # step 4: four queries, two in each query block, take every eligible row: a tile's 256 rows times four queries go
    # through the waves' hit logs into the 512-entry spill regions, which fill and are worked off inside the launch
    everything = [0, 100, 256, NQ - 1]
    thr = thr.copy()
    thr[everything] = worse(p.cfg.metric)
    counts, st = range_search(p, rq, thr, "step 4: four thresholds at infinity")
    assert (counts[everything] == m.live_count()).all() and (counts >= K).all(), counts[everything]
    assert st["fallback_queries"] == 0 and np.isfinite(st["eps_bound"]) and st["max_fast_err"] <= st["eps_bound"], st


def phase_byid(p, n):
    """Steps 5 - 6: 300 gathered queries with the row itself excluded, the graph of the first 600 rows."""
    m = p.model
    delete(p, n)
    rng = np.random.default_rng(7200 + p.cfg.dim)
    live = np.flatnonzero(~m.deleted)
    ids = np.concatenate([live[[0, -1]], rng.choice(live[1:-1], NQ - 2, replace=False)]).astype(np.uint64) + np.uint64(m.offset)
    p.routed(S.Op("search_by_ids", dict(ids=ids, k=K, exclude_self=True)), PATH_MFMA, "step 5: 300 ids")
    assert 256 < int(m.deleted[:600].sum()) < 600
    st = p.routed(S.Op("knn_graph", dict(k=K, first_id=m.offset, n=600)), PATH_MFMA, "step 6: the graph of rows 0 .. 599")
    assert st["nq"] == 600 - int(m.deleted[:600].sum()) > 64, st


def phase_filtered(p, n):
    """Steps 7 - 8: the allow list beside the tombstones, then labelled and grouped searches on their dense route."""
    m = p.model
    delete(p, n)
    set_allow_list(p, n)
    rq = queries(p, 7, NQ)
    search(p, rq, K, "step 7: under the allow list")
    counts, _ = range_search(p, rq, p.rank_thresholds(rq, K), "step 7: range under the allow list")
    assert (counts >= K).all(), counts[counts < K]
    set_label_plan(p, n)
    # with the path forced every label is answered by a dense scan under its mask; the big label's 260 queries fill two
    # query blocks of the 4-wave kernel
    ql = np.array([L_BIG] * 260 + [0] * 20 + [L_SMALL + j for j in range(N_SMALL)] * 4 + [S.L_NOBODY] * 4, np.uint32)
    assert ql.size == NQ
    rq = queries(p, 8, NQ)
    p.routed(S.Op("search_labeled", dict(rq=rq, k=K, qlabels=ql)), PATH_MFMA, "step 8: labelled")
    # grouped, k = 2: the big label and label 0 share every query's first list, so the candidate search (300 queries,
    # k' rows each) answers alone; k = 3: most queries need the dense stage behind it
    p.routed(S.Op("search_grouped", dict(rq=rq, k=2)), PATH_MFMA, "step 8: grouped, k = 2")
    p.check(S.Op("search_grouped", dict(rq=rq, k=3)), "step 8: grouped, k = 3")
    assert p.ix.last_stats()["path"] in (PATH_MFMA, PATH_EXACT), p.ix.last_stats()


def chain(p, batches, k):
    """Step 11: pipelined searches, two in flight, over two sets of device buffers (Pair.pipeline is fixed at 3 queries,
    the stream route).  Every launch reuses its slot's pacing and claim regions behind their memsets."""
    torch, ix = p.torch, p.ix
    nq, dim = batches[0].shape
    dq = [torch.empty((nq, dim), dtype=torch.float32, device=p.dev) for _ in range(2)]
    out = [(torch.empty((nq, k), dtype=torch.int64, device=p.dev), torch.empty((nq, k), dtype=torch.float32, device=p.dev)) for _ in range(2)]

    def begin(s):
        dq[s % 2].copy_(torch.from_numpy(np.ascontiguousarray(batches[s])))
        torch.cuda.synchronize()
        ix.search_begin_device(dq[s % 2], k, *out[s % 2])
    begin(0)
    for s in range(len(batches)):
        if s + 1 < len(batches):
            begin(s + 1)
            assert ix.pending == 2
        ix.search_end()
        st = ix.last_stats()
        assert st["path"] == PATH_MFMA and st["nq"] == nq, (s, st)
        got = (out[s % 2][0].cpu().numpy().view(np.uint64).copy(), out[s % 2][1].cpu().numpy().copy())
        same_lists(got, p.model.search(batches[s], k), f"{p.cfg.name}: search {s} of the pipelined chain")
    assert ix.pending == 0


def phase_rewritten(p, n):
    """Steps 9 - 11: rows updated in place, compaction under the tombstones, the allow list and the labels, and a chain
    of pipelined searches; then the handle grown into the staged form."""
    m = p.model
    delete(p, n)
    set_allow_list(p, n)
    set_label_plan(p, n)
    rng = np.random.default_rng(7300 + p.cfg.dim)
    live = np.flatnonzero(~m.deleted)
    touched = np.concatenate([live[[0, -1]], rng.choice(live[1:-1], 48, replace=False)])
    new = p.fresh_rows(50)
    p.update(touched, new)
    p.read_back(touched, "step 9")
    search(p, np.concatenate([new, queries(p, 9, NQ - 50)]), K, "step 9: 50 of the queries are the new rows")
    dead = int(m.deleted.sum())
    p.compact()                                                     # (Pair compares the new-id map with the model's)
    assert m.count == n - dead and m.count % 256 != 0
    search(p, queries(p, 10, NQ), K, "step 10: after the compaction")
    chain(p, [queries(p, 20 + s, NQ) for s in range(6)], K)
    # step 12: past 8192 rows the search is staged -- a sample launch, under a mask in its every-score form, and two
    # filtered launches, the last one ending on a partial tile; the new rows are not on the allow list
    p.add(p.fresh_rows(GROWN_ROWS - m.count))
    metric, cus = plan_metric(p.cfg.metric), _cus()
    assert m.count == GROWN_ROWS > LIST_CAP and GROWN_ROWS % 256 != 0 and len(stage_plan(GROWN_ROWS, NQ, K, metric, cus)[2]) == 2
    for k, tag in ((K, "step 12: staged, k = 10"), (100, "step 12: staged, k = 100")):
        st = search(p, queries(p, 30 + k, NQ), k, tag)
        kp, sample, _ = stage_plan(GROWN_ROWS, NQ, k, metric, cus)
        assert not sample_is_grouped(sample, kp), (sample, kp)
        want = scan_launches(GROWN_ROWS, NQ, k, p.cfg.metric, cus)
        assert st["scan_launches"] == want if st["fallback_queries"] == st["band_queries"] == 0 else st["scan_launches"] >= want, (tag, st, want)


RUN = dict(plain=phase_plain, deleted=phase_deleted, byid=phase_byid, filtered=phase_filtered, rewritten=phase_rewritten)


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("dim", list(WIDTHS))
def test_handle_script(va, dim, phase):
    kt, tile_loop, metric, id_offset, n = WIDTHS[dim]
    assert k_tiles(dim) == kt and takes_tile_loop(dim) == tile_loop
    cfg = S.Config(f"w4-{dim}-bf16-{metric}", dim, "bf16", metric, id_offset=id_offset)
    with Pair(va, cfg, 8000 + dim) as p:
        build(p, n)
        RUN[phase](p, n)


# ================================================================ B: tile-range endings under a mask and under range search
B_CASES = [(d, m) for d in B_DIMS for m in METRICS]


@pytest.fixture(scope="module", params=B_CASES, ids=[f"{d}-{m}" for d, m in B_CASES])
def world(request, oracle):
    """The oracle side of one (dim, metric), computed once: every query's full ranking (one oracle call), the mask -- a
    whole tile, every third row of 20 tiles and each query's unmasked top-10 deleted, 30 % more dropped by the allow
    list -- and the best-first scores of the eligible rows and of all rows."""
    dim, metric = request.param
    rng = np.random.default_rng(100 * dim + METRICS.index(metric))
    raw = oracle.synth_rows(81, 0, B_N, dim, threads=THREADS)
    rq = oracle.synth_rows(82, 0, NQ, dim, threads=THREADS)
    if metric == "ip":                                             # norms spread over 0.5 .. 2, so that ip is not cosine
        raw = (raw * rng.uniform(0.5, 2.0, (B_N, 1))).astype(np.float32)
        rq = (rq * rng.uniform(0.5, 2.0, (NQ, 1))).astype(np.float32)
    lims, ids, sc = oracle.range_search(raw, rq, worse(metric), DT["bf16"], prep_of(metric), form_of(metric), threads=THREADS)
    assert np.array_equal(lims, np.arange(NQ + 1, dtype=np.uint64) * np.uint64(B_N))
    ids, sc = ids.reshape(NQ, B_N).astype(np.int64), sc.reshape(NQ, B_N)
    top10 = ids[:, :K].copy()
    dead = np.unique(np.concatenate([np.arange(7 * 256, 8 * 256), np.arange(100 * 256, 120 * 256, 3), top10.ravel()]))
    allow = rng.random(B_N) >= 0.3
    mask = allow.copy()
    mask[dead] = False
    keep = mask[ids]
    m = int(mask.sum())
    assert (keep.sum(axis=1) == m).all() and 0.6 * B_N < m < 0.72 * B_N
    cut = 20_001
    return dict(dim=dim, metric=metric, raw=raw, rq=rq, top10=top10, dead=dead, allow=allow, mask=mask,
                s_all=sc[:, :cut].copy(), s_masked=sc[keep].reshape(NQ, m)[:, :cut].copy())


def b_handle(va, w, masked):
    ix = va.Index(w["dim"], "bf16", w["metric"])
    ix.add(w["raw"])
    ix.set_path(PATH_MFMA)
    if masked:
        ix.delete(w["dead"])
        ix.set_filter(w["allow"])
    return ix


def assert_b_shape(dim, metric):
    assert takes_tile_loop(dim)
    _, _, lens = stage_strip_lens(B_N, NQ, K, plan_metric(metric), _cus())
    assert 1 in lens[-1] and 2 in lens[-1] and max(lens[-1]) == 2, lens[-1]   # static ranges of exactly one and exactly two tiles
    assert B_N % 256 != 0                                                     # ... and a partial last tile
    return lens


def test_masked_topk_at_one_and_two_tile_ranges(va, oracle, world):
    w = world
    dim, metric = w["dim"], w["metric"]
    lens = assert_b_shape(dim, metric)
    elig = eligible_rows(B_N, w["allow"], w["dead"])
    assert np.array_equal(elig, np.flatnonzero(w["mask"]))
    assert not np.isin(w["top10"], elig).any()                     # every query's unmasked top-10 is wholly ineligible
    want = oracle_over(oracle, w["raw"], w["rq"], K, "bf16", metric, elig)
    with b_handle(va, w, True) as ix:
        ids, sc = ix.search(w["rq"], K)
        st = ix.last_stats()
    print(dim, metric, st)
    assert st["path"] == PATH_MFMA and len(lens) == 2, (st, lens)
    assert st["scan_launches"] == 3 if st["fallback_queries"] == st["band_queries"] == 0 else st["scan_launches"] >= 3, st   # the restated plan is the library's
    assert_same_all_bits(ids, sc, *want, f"masked top-k {dim}/{metric}")
    assert w["mask"][ids.astype(np.int64)].all()


def b_thresholds(s, metric):
    """hard_thresholds (rank 1, 10, 1000, a midpoint, nothing), then: queries 5 and 261 at rank 9000 and queries 6 and 262
    at rank 20 000 -- more than a list, so their rows are redone in pieces, in both query blocks -- query 11 at the
    infinity every row reaches and query 289 at the one no row reaches."""
    thr = hard_thresholds(s, metric)
    for q, rank in ((5, 9000), (261, 9000), (6, 20_000), (262, 20_000)):
        thr[q] = s[q, rank - 1]
    thr[11], thr[289] = worse(metric), -worse(metric)
    return thr


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
def test_range_search_at_one_and_two_tile_ranges(va, oracle, world, masked):
    w = world
    dim, metric = w["dim"], w["metric"]
    assert_b_shape(dim, metric)
    thr = b_thresholds(w["s_masked"] if masked else w["s_all"], metric)
    mask = w["mask"] if masked else None
    want = oracle.range_search(w["raw"], w["rq"], thr, DT["bf16"], prep_of(metric), form_of(metric), mask=mask, threads=THREADS)
    with b_handle(va, w, masked) as ix:
        lims, ids, sc = ix.range_search(w["rq"], thr)
        st = ix.last_stats()
    what = f"range {dim}/{metric}/{'masked' if masked else 'unmasked'}"
    print(what, st, "total", int(lims[-1]))
    assert np.array_equal(lims, want[0]), f"{what}: counts differ at queries {np.flatnonzero(np.diff(lims.astype(np.int64)) != np.diff(want[0].astype(np.int64)))[:8]}"
    assert_same_all_bits(ids, sc, want[1], want[2], what)
    counts = np.diff(want[0].astype(np.int64))
    rows = int(w["mask"].sum()) if masked else B_N
    assert counts[0] >= 1 and counts[1] >= 10 and counts[2] >= 1000 and counts[3] == 21 and counts[4] == 0, counts[:5]
    assert (counts[[5, 261]] >= 9000).all() and (counts[[6, 262]] >= 20_000).all() and counts[11] == rows and counts[289] == 0, counts[[5, 261, 6, 262, 11, 289]]
    assert counts[5] > LIST_CAP and st["scan_launches"] > 1, (what, st)                   # redone in pieces
    assert st["path"] == PATH_MFMA and st["fallback_queries"] == 0, (what, st)
    assert np.isfinite(st["eps_bound"]) and st["max_fast_err"] <= st["eps_bound"], (what, st)


def test_more_query_blocks_than_work_group_slots_under_the_tile_loop(va, oracle):
    """33 query blocks over 2003 rows at dim 256: a work-group takes one query block, so a device of 256 CUs (32 slots)
    runs every stage as two kernel launches, the second with qb_base = 32 and a single, partial-free query block."""
    dim = 256
    assert takes_tile_loop(dim) and B_MANY_NQ == 33 * 256 and B_MANY_ROWS % 256 != 0
    assert 256 * (_cus() // 8) < B_MANY_NQ, _cus()
    raw = oracle.synth_rows(83, 0, B_MANY_ROWS, dim, threads=THREADS)
    rq = oracle.synth_rows(84, 0, B_MANY_NQ, dim, threads=THREADS)
    oi, osc = oracle.search(raw, rq, K, DT["bf16"], 0, threads=THREADS)
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        ids, sc = ix.search(rq, K)
        st = ix.last_stats()
    print(st)
    assert st["path"] == PATH_MFMA and st["nq"] == B_MANY_NQ, st
    assert_same_all_bits(ids, sc, oi, osc, "33 query blocks")


# ================================================================ C: pacing points inside the tile loop
_PACE_CODE = r'''
import sys, numpy as np, torch
sys.path.insert(0, ".")
import vrod_amd as va
dim, n, nq, k = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
ix = va.Index(dim, "bf16", "cosine"); ix.add_synthetic(1, 0, n); ix.set_path(va.PATH_MFMA)
oi = torch.empty((nq, k), dtype=torch.int64, device="cuda"); osc = torch.empty((nq, k), dtype=torch.float32, device="cuda")
ix.search_synthetic_device(2, 0, nq, k, oi, osc); torch.cuda.synchronize()
assert ix.last_stats()["path"] == va.PATH_MFMA, ix.last_stats()
np.save(sys.argv[1], np.concatenate([oi.cpu().numpy().astype(np.int64), osc.cpu().numpy().view(np.int32).astype(np.int64)], axis=1))
'''


@pytest.mark.parametrize("dim", C_DIMS)
def test_pacing_settings_give_the_same_bits(dim):
    """At the default interval (192 K-tiles) no small shape reaches a pacing point under the tile loop; at 8 K-tiles the
    countdown fires at the third tile of every 4- or 5-tile range, with the two query blocks' work-groups at the
    counter.  Pacing moves no result: off, the default and 8 give the same ids and score bits."""
    kt = k_tiles(dim)
    assert takes_tile_loop(dim)
    _, _, lens = stage_strip_lens(C_N, NQ, K, "cosine", _cus())
    assert set(lens[-1]) == {4, 5}, set(lens[-1])
    assert tloop_pace_tiles(kt, 8, 4)[:1] == [3] and not tloop_pace_tiles(kt, 192, 5) and not tloop_pace_tiles(kt, 0, 5)
    outs = []
    for setting in C_SETTINGS:
        path = f"/tmp/vrod_w4_forms_pace_{os.getpid()}_{dim}_{setting}.npy"
        env = dict(os.environ)
        env.pop("VROD_DEBUG_PACE_KT", None)
        if setting is not None:
            env["VROD_DEBUG_PACE_KT"] = setting
        r = subprocess.run([sys.executable, "-c", _PACE_CODE, path, str(dim), str(C_N), str(NQ), str(K)], capture_output=True, text=True,
                           cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, (setting, r.stderr[-2000:])
        outs.append(np.load(path))
        os.unlink(path)
    assert outs[0].shape == (NQ, 2 * K)
    for setting, got in zip(C_SETTINGS[1:], outs[1:]):
        assert np.array_equal(got, outs[0]), f"VROD_DEBUG_PACE_KT={setting} differs from the default at {np.argwhere(got != outs[0])[:5].tolist()}"


def test_default_pacing_at_dim_384_equals_the_oracle(va, oracle):
    """The default of the comparison above against the oracle (dim 256: test_gpu_w4_tile_loop.test_group_best_sample_form)."""
    dim = 384
    raw = oracle.synth_rows(1, 0, C_N, dim, threads=THREADS)
    rq = oracle.synth_rows(2, 0, NQ, dim, threads=THREADS)
    oi, osc = oracle.search(raw, rq, K, DT["bf16"], 0, threads=THREADS)
    assert os.environ.get("VROD_DEBUG_PACE_KT") is None
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_path(PATH_MFMA)
        ids, sc = ix.search(rq, K)
        st = ix.last_stats()
    assert st["path"] == PATH_MFMA, st
    assert_same_all_bits(ids, sc, oi, osc, "170 000 x 384, default pacing")
