"""Long-lived handles: sequences of operations on ONE handle, every step applied to a plain-Python model as well
(index_model.ModelIndex) and every search form compared with the model bit for bit (sequence_exec.Pair).

test_random_sequences runs the eight committed plans of sequence_plans.py (what they reach is asserted on a CPU by
test_sequence_plans.py, which routes every search as search_plan.h does).  The scripted orderings below are short and deterministic, each named after the piece of
per-handle state it pins, so that a failure of a random plan can be reduced to one of them.
"""
import ctypes as C

import numpy as np
import pytest

import sequence_plans as S
from sequence_exec import ERR_UNSUPPORTED, SENT_ID, SENT_SC, Pair, same_lists
from support import PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_GATHER

pytestmark = pytest.mark.gpu

D = 72
L_BIG, L_NOBODY = S.L_BIG, S.L_NOBODY


@pytest.fixture(scope="module")
def va(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import vrod_amd
    vrod_amd.load()
    return vrod_amd


def rows(rng, n, d=D):
    return rng.standard_normal((n, d)).astype(np.float32)


def labelling(rng, n):
    """A label on more than half of the rows, labels of 20 rows on a quarter of them, label 0 on the rest."""
    lab = np.zeros(n, np.uint32)
    perm = rng.permutation(n)
    big = n // 2 + 10
    lab[perm[:big]] = L_BIG
    for j in range(n // 80):
        lab[perm[big + 20 * j:big + 20 * j + 20]] = S.L_SMALL0 + j
    return lab


@pytest.mark.parametrize("seed,cfg", S.COMMITTED, ids=[f"{seed}-{cfg.name}" for seed, cfg in S.COMMITTED])
def test_random_sequences(va, seed, cfg):
    with Pair(va, cfg, seed) as p:
        p.run_plan(S.make_plan(seed, cfg))


# ---------------------------------------------------------------------------------- scripted orderings
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_growth_with_tombstones_filter_and_labels(va, dtype):
    cfg = S.Config(f"growth-{dtype}", D, dtype, "cosine")
    rng = np.random.default_rng(101)
    with Pair(va, cfg, 101) as p:
        p.add(rows(rng, 300))                                   # capacity 512
        assert p.model.capacity == 512
        for size in (400, 700):                                 # 700 rows -> 768, 1 400 rows -> 1 536: the second growth starts from a grown state
            n = p.model.count
            p.delete(rng.choice(np.flatnonzero(~p.model.deleted), n // 10, replace=False))
            p.set_filter(rng.random(n) < 0.5)
            p.set_labels(0, labelling(rng, n))
            cap = p.model.capacity
            p.add(rows(rng, size))
            assert p.model.capacity > cap                       # a reallocation
            assert not p.model.eligible()[n:].any() and (p.model.labels[n:] == 0).all()
            assert (p.ix.get_labels(n, size) == 0).all()
            got = p.ix.search(p.model.rows[n:n + 5], 1)[0]      # the new rows themselves as queries: none of them comes back
            assert (got < np.uint64(n)).all()
            p.check_every_form(f"after the growth by {size}", nqs=(3, 40))
            p.set_filter(None)
            p.check_every_form(f"after the growth by {size}, filter cleared", nqs=(3, 40))


@pytest.mark.parametrize("split", ["1", None])
def test_update_of_rows_the_planes_do_not_cover(va, split):
    cfg = S.Config(f"planes-{split}", D, "f32", "l2", split=split)
    rng = np.random.default_rng(202)

    def batched(tag):
        for nq in (40, 300):
            for path in (PATH_AUTO, PATH_MFMA):
                p.ix.set_path(path)
                p.check(S.Op("search", dict(rq=rows(rng, nq), k=10)), f"{tag} nq {nq} path {path}")
        p.ix.set_path(PATH_AUTO)

    def add_update_search(n_new, tag):
        old = p.model.count
        cap = p.model.capacity
        p.add(rows(rng, n_new))
        live = np.flatnonzero(~p.model.deleted)
        touched = np.concatenate([rng.choice(live[live < old], 30, replace=False), rng.choice(live[live >= old], min(30, n_new), replace=False)])
        touched = np.concatenate([touched, touched[:2]])        # (two ids twice: the last vector stays)
        p.update(touched, rows(rng, touched.size))
        batched(tag)
        # the updated rows are found by their new vectors
        q = p.model.rows[touched[:8]]
        assert (p.ix.search(q, 1)[0][:, 0] == touched[:8].astype(np.uint64)).all(), tag
        return p.model.capacity > cap

    with Pair(va, cfg, 202) as p:
        p.add(rows(rng, 1000))                                  # capacity 1024
        batched("planes built")
        assert not add_update_search(20, "an add within the capacity")
        assert add_update_search(300, "an add that grows the capacity")
        p.delete(np.arange(100, 400))
        p.compact()
        assert not add_update_search(50, "after a compaction")
        p.check_every_form("at the end", nqs=(40,))


def test_rows_added_after_a_compaction_start_clean(va):
    cfg = S.Config("after-compaction", D, "bf16", "ip", id_offset=5_000_000_000)
    rng = np.random.default_rng(303)
    L_TAIL = 4242
    with Pair(va, cfg, 303) as p:
        n, tail = 1500, 200
        p.add(rows(rng, n))
        lab = labelling(rng, n)
        lab[n - tail:] = L_TAIL
        p.set_labels(0, lab)
        allow = rng.random(n) < 0.3
        allow[n - tail:] = True
        p.set_filter(allow)
        p.delete(np.arange(n - tail, n))
        p.compact()
        new = rows(rng, tail + 50)
        p.add(new)
        m = p.model
        first = n - tail
        assert (p.ix.get_labels(cfg.id_offset + first, tail + 50) == 0).all()
        q = np.concatenate([new[:6], rows(rng, 3)])
        ids, sc = p.ix.search_labeled(q, 10, np.full(9, L_TAIL, np.uint32))
        assert (ids == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and np.isnan(sc).all()
        assert p.ix.filter_count() == int(allow[:first].sum())
        assert (p.ix.search(new[:6], 5)[0] < np.uint64(cfg.id_offset + first)).all()    # not allowed while the filter stands
        p.check_every_form("new rows under the old filter", nqs=(3, 40))
        p.set_filter(None)
        ids, _ = p.ix.search_labeled(q, 10, np.full(9, L_TAIL, np.uint32))
        assert (ids == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
        p.check_every_form("new rows, filter cleared", nqs=(3, 40))
        assert m.count == first + tail + 50


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mask_override_leaves_the_caches_alone(va, dtype):
    cfg = S.Config(f"override-{dtype}", D, dtype, "cosine", split="1" if dtype == "f32" else None)
    rng = np.random.default_rng(404)
    n = 3000
    with Pair(va, cfg, 404) as p:
        p.add(rows(rng, n))
        p.set_labels(0, labelling(rng, n))
        p.delete(rng.choice(n, 100, replace=False))
        narrow = rng.random(n) < 0.02
        qlab = np.array([L_BIG, S.L_SMALL0 + 3, L_NOBODY, L_BIG, 0, S.L_SMALL0 + 7], np.uint32)
        near_big = p.model.rows[np.flatnonzero(p.model.labels == L_BIG)[:4]] + 0.01 * rows(rng, 4)   # the best ranks: one label

        def triple(search_op, tag):
            first = p.check(search_op, f"{tag}: before")
            p.check(S.Op("search_labeled", dict(rq=rows(rng, 6), k=10, qlabels=qlab)), tag)
            p.check(S.Op("search_grouped", dict(rq=near_big, k=40)), tag)       # more labels than its first list holds: the dense stage
            again = p.check(search_op, f"{tag}: after")
            assert np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32)), tag

        p.set_filter(narrow)
        p.set_path(PATH_GATHER)
        gather = S.Op("search", dict(rq=rows(rng, 9), k=10))
        triple(gather, "the gather list")
        # another filter with as many eligible rows: the list must follow the mask, not its size
        live = ~p.model.deleted
        moved = narrow.copy()
        moved[narrow & live] = False
        moved[rng.choice(np.flatnonzero(~narrow & live), int((narrow & live).sum()), replace=False)] = True
        p.set_filter(moved)
        assert p.model.filter_count() == int((narrow & ~p.model.deleted).sum())
        p.check(gather, "the gather list after a filter of the same size")
        # the sample window of a forced-MFMA batch under a broad filter
        p.set_filter(rng.random(n) < 0.5)
        p.set_path(PATH_MFMA)
        triple(S.Op("search", dict(rq=rows(rng, 300), k=10)), "the sample window")
        # a delete and an add that leave the eligible count as it was, no filter: the list again
        p.set_filter(None)
        p.set_path(PATH_GATHER)
        p.check(gather, "no filter")
        p.delete([int(p.check(gather)[0][0, 0])])
        p.add(rows(rng, 1))
        p.check(gather, "one row deleted, one added")


def test_graph_replay_around_the_other_entry_points(va):
    cfg = S.Config("replay", D, "f32", "cosine", split="0")
    rng = np.random.default_rng(505)
    n = 2000
    with Pair(va, cfg, 505) as p:
        p.add(rows(rng, n))
        p.set_labels(0, labelling(rng, n))
        p.delete(rng.choice(n, 50, replace=False))

        def chain(tag):
            p.check(S.Op("pipelined", dict(rq=rows(rng, S.PIPE_CHAIN * S.PIPE_NQ).reshape(S.PIPE_CHAIN, S.PIPE_NQ, D), k=S.PIPE_K)), tag)
            return p.ix.last_stats()

        # Nothing the C ABI reports tells a replayed search from plainly launched ones (a replay restores the counters of
        # the search it captured, which are a plain search's): that the chain reaches the replay branch follows from
        # search_enqueue alone -- a forced stream path, 3 queries, a search pending, the same buffers in each slot: plain,
        # capture, replay.  What is asserted is that the counters survive whichever way the launches went.
        p.set_path(PATH_STREAM)
        p.ix.search(rows(rng, S.PIPE_NQ), S.PIPE_K)
        plain = p.ix.last_stats()                               # the same search, begun with nothing pending: never captured
        st = chain("first chain: plain, capture, replay")
        assert st["scan_launches"] == plain["scan_launches"] and st["nq"] == S.PIPE_NQ and st["k"] == S.PIPE_K, (st, plain)
        others = [S.Op("search_labeled", dict(rq=rows(rng, 5), k=10, qlabels=np.array([L_BIG, S.L_SMALL0, L_NOBODY, 0, L_BIG], np.uint32))),
                  S.Op("search_grouped", dict(rq=rows(rng, 5), k=10)),
                  S.Op("range_search", dict(rq=rows(rng, 5), thr=np.full(5, 0.2, np.float32))),
                  S.Op("search_by_ids", dict(ids=np.flatnonzero(~p.model.deleted)[:7].astype(np.uint64), k=10, exclude_self=True)),
                  S.Op("knn_graph", dict(k=5, first_id=None, n=None))]
        for op in others:
            p.check(op)
            st = chain(f"after {op.kind}")
            assert st["scan_launches"] == plain["scan_launches"], (op.kind, st)
            live = np.flatnonzero(~p.model.deleted)
            p.update(rng.choice(live, 40, replace=False), rows(rng, 40))
            chain(f"after {op.kind} and an update")


def test_two_shard_handle_sequence(va):
    d, n = 32, 140_000
    cfg = S.Config("two-shards", d, "bf16", "cosine")
    rng = np.random.default_rng(606)
    with Pair(va, cfg, 606, devices=[0, 0]) as p:
        forms = ("search", "range_search", "pipelined")
        p.add(rows(rng, 65_000, d))
        p.add(rows(rng, n - 65_000, d))                          # across the 65 536-row block boundary: both shards hold rows
        p.check_every_form("both shards", nqs=(3,), forms=forms)
        p.delete(np.concatenate([np.arange(65_530, 65_542), np.arange(131_068, 131_076), rng.choice(n, 3000, replace=False)]))
        p.check_every_form("deleted", nqs=(3,), forms=forms)
        live = np.flatnonzero(~p.model.deleted)
        touched = np.concatenate([rng.choice(live, 60, replace=False), live[(live > 65_500) & (live < 65_600)][:10]])
        p.update(touched, rows(rng, touched.size, d))
        p.check_every_form("updated", nqs=(9,), forms=forms)
        p.set_filter(rng.random(n - 1000) < 0.3)
        p.check_every_form("filtered", nqs=(3,), forms=forms)
        p.add(rows(rng, 37, d))
        p.check_every_form("rows added under the filter", nqs=(3,), forms=forms)
        # what a composite handle does not support says so, writes nothing and changes nothing
        ix = p.ix
        buf = np.full(p.model.count, SENT_ID, np.uint64)
        assert ix._L.vrod_index_compact(ix._h, buf.ctypes.data_as(C.c_void_p), buf.size) == ERR_UNSUPPORTED and (buf == SENT_ID).all()
        q = rows(rng, 3, d)
        for call in (lambda: ix.set_labels(0, np.ones(10, np.uint32)), lambda: ix.search_labeled(q, 5, np.zeros(3, np.uint32)),
                     lambda: ix.search_grouped(q, 5), lambda: ix.search_by_ids([1, 2], 5), lambda: ix.knn_graph(5, first_id=0, n=8)):
            p.raises(ERR_UNSUPPORTED, call, "a composite handle")
        oi = np.full((2, 5), SENT_ID, np.uint64)
        sc = np.full((2, 5), SENT_SC, np.float32)
        ids = np.array([1, 2], np.uint64)
        assert ix._L.vrod_search_by_ids(ix._h, ids.ctypes.data_as(C.c_void_p), 2, 5, 0, oi.ctypes.data_as(C.c_void_p),
                                        sc.ctypes.data_as(C.c_void_p)) == ERR_UNSUPPORTED
        assert (oi == SENT_ID).all() and (sc == SENT_SC).all()
        assert (ix.get_labels(0, 10) == 0).all()
        p.state("after the unsupported calls")
        same_lists(ix.search(q, 10), p.model.search(q, 10), "the search right after the unsupported calls")
        p.set_filter(None)
        p.check_every_form("filter cleared", nqs=(3,), forms=forms)
