"""CPU tests of the sequence plans (sequence_plans.py) and of the handle model (index_model.py).

1. Every committed (seed, config) reaches the orderings the plans exist for.  These are conditions, not measurements: a
   change of the generator after which a plan no longer reaches one of them fails here instead of thinning out quietly.
2. The model is right: for the three small plans (one of them at the odd width 33) every check op's expected values are compared with an independent numpy
   restatement -- oracle.numpy_prepare, numpy_scores_canonical over the FULL row set, a mask instead of a gathered subset,
   numpy_topk_from_scores / numpy_range_from_scores -- in ids and score bits.  To keep the CPU suite quick two kinds of
   check op are sampled, not compared whole: of a pipelined op's 8 searches (all of them model.search, which the plain
   search ops compare in full) the first 2, and of a knn_graph 48 random rows, deleted ones among them.
"""
import numpy as np
import pytest

import sequence_plans as S
from index_model import ID_NONE, ModelIndex
from support import bits
from oracle import oracle as O

PLANS = {}


def plan_of(seed, cfg):
    if (seed, cfg) not in PLANS:
        PLANS[(seed, cfg)] = S.make_plan(seed, cfg)
    return PLANS[(seed, cfg)]


EVERY = S.COMMITTED + S.MODEL_CHECK
IDS = [f"{seed}-{cfg.name}" for seed, cfg in EVERY]


@pytest.mark.parametrize("seed,cfg", EVERY, ids=IDS)
def test_every_committed_plan_reaches_the_orderings(oracle, seed, cfg):
    plan = plan_of(seed, cfg)
    again = S.make_plan(seed, cfg)
    assert [repr(a) for a in plan] == [repr(b) for b in again] and all(
        x.tobytes() == y.tobytes() for a, b in zip(plan, again) for x, y in zip(a.a.values(), b.a.values()) if isinstance(x, np.ndarray)), "not deterministic"
    cov = S.coverage(plan, cfg)
    assert cov["a"] >= 2, "capacity growths while tombstones, a filter and labels all exist"
    assert cov["b"] >= 1, "a compaction with a filter and labels set"
    assert cov["c"] >= 1, "an add after a compaction"
    assert cov["f"] >= 3, "rejected ops"
    if cfg.dtype == "f32" and cfg.split != "0":         # (VROD_F32_SPLIT=0: a handle without planes)
        assert cov["d"] >= 1, "an update on both sides of the rows the planes cover, the planes built by a split MFMA batch"
    assert cov["g"] >= 1, "gather search, labelled search, gather search with no mask change between"
    assert sum(cov["h"].values()) >= 2, "graphable pipelined chains behind two of the labelled / grouped / range / by-id searches, a graphable chain before each"
    assert cov["k_above"] >= 1, "a k above the eligible rows"
    assert cov["knn"] <= S.KNN_PER_PLAN
    assert 30 <= cov["steps"] <= 41, cov["steps"]
    if cfg.small:                                       # (sequence_plans' docstring: why these are smaller than the issue's sizes)
        assert cov["max_rows"] <= 2000
    else:
        assert 1500 <= cov["final_rows"] and cov["max_rows"] <= S.MAX_ROWS
        assert cov["labellings"] >= 1, "a labelling with a label on most rows, 40 small labels, label 0 and an unused label"


def test_the_committed_set_puts_every_form_behind_every_mutation(oracle):
    cells, h = {}, {}
    for seed, cfg in S.COMMITTED:
        cov = S.coverage(plan_of(seed, cfg), cfg)
        for key, n in cov["e"].items():
            cells[key] = cells.get(key, 0) + n
        for key, n in cov["h"].items():
            h[key] = h.get(key, 0) + n
    missing = [(form, kind) for form in S.FORMS for kind in S.MUTATIONS if cells.get((form, kind), 0) < 1]
    assert not missing, missing
    assert all(n >= 1 for n in h.values()), h
    dims = {cfg.dim for _, cfg in S.COMMITTED}
    assert dims == {64, 72, 100}
    assert {(cfg.dtype, cfg.metric) for _, cfg in S.COMMITTED} >= {(t, m) for t in ("f32", "bf16") for m in ("cosine", "l2", "ip")}
    assert {cfg.split for _, cfg in S.COMMITTED if cfg.dtype == "f32"} == {"0", "1", None}
    assert sum(1 for _, cfg in S.COMMITTED if cfg.id_offset) == 2
    assert len(S.COMMITTED) == 8 and not any(cfg.small for _, cfg in S.COMMITTED)


# ---------------------------------------------------------------------------------- the model against numpy
def numpy_lists(m, pq, k, elig, drop=None):
    """Top-k from the canonical scores of EVERY row: the ineligible rows are given the worst score, and a slot that one
    of them still reaches is unfilled.  drop: per query a local row that is no candidate (the query's own row)."""
    pc = O.numpy_prepare(m.rows, {"f32": 0, "bf16": 1}[m.dtype], m.prep)
    sc = O.numpy_scores_canonical(pc, pq, m.form)
    worst = np.float32(np.inf) if m.form == 1 else np.float32(-np.inf)
    ok = np.broadcast_to(elig, sc.shape).copy()
    if drop is not None:
        ok[np.arange(sc.shape[0]), drop] = False
    assert np.isfinite(sc).all()
    masked = np.where(ok, sc, worst)
    ids, s = O.numpy_topk_from_scores(masked, k, m.form, id_offset=m.offset)
    loc = np.where(ids == ID_NONE, 0, ids - np.uint64(m.offset)).astype(np.int64)
    bad = (ids == ID_NONE) | ~np.take_along_axis(ok, loc, axis=1)
    return np.where(bad, ID_NONE, ids), np.where(bad, np.float32(np.nan), s)


def numpy_expected(m, op):
    a = op.a
    dt = {"f32": 0, "bf16": 1}[m.dtype]
    elig = m.eligible()
    if op.kind in ("search", "search_labeled", "search_grouped", "range_search"):
        pq = O.numpy_prepare(a["rq"], dt, m.prep)
    if op.kind == "search":
        return numpy_lists(m, pq, a["k"], elig)
    if op.kind == "search_labeled":
        ids = np.empty((pq.shape[0], a["k"]), np.uint64)
        sc = np.empty((pq.shape[0], a["k"]), np.float32)
        for q in range(pq.shape[0]):
            ids[q], sc[q] = (x[0] for x in numpy_lists(m, pq[q:q + 1], a["k"], elig & (m.labels == a["qlabels"][q])))
        return ids, sc
    if op.kind == "search_grouped":
        k, nq = a["k"], pq.shape[0]
        present = np.unique(m.labels[elig])
        reps = [numpy_lists(m, pq, 1, elig & (m.labels == L)) for L in present]
        oi = np.full((nq, k), ID_NONE, np.uint64)
        osc = np.full((nq, k), np.nan, np.float32)
        ol = np.zeros((nq, k), np.uint32)
        for q in range(nq):
            items = sorted(((float(r[1][q, 0]) * (1 if m.form == 1 else -1), int(r[0][q, 0]), int(L)) for r, L in zip(reps, present)))[:k]
            for j, (_, i, L) in enumerate(items):
                oi[q, j], ol[q, j] = i, L
                osc[q, j] = reps[list(present).index(L)][1][q, 0]
        return oi, osc, ol
    if op.kind == "range_search":
        pc = O.numpy_prepare(m.rows, dt, m.prep)
        return O.numpy_range_from_scores(O.numpy_scores_canonical(pc, pq, m.form), a["thr"], m.form, mask=elig, id_offset=m.offset)
    if op.kind == "search_by_ids":
        loc = (np.asarray(a["ids"], np.uint64) - np.uint64(m.offset)).astype(np.int64)
        pq = O.numpy_prepare(m.rows, dt, m.prep)[loc]
        return numpy_lists(m, pq, a["k"], elig, drop=loc if a["exclude_self"] else None)
    raise ValueError(op.kind)


SMALL = list(S.MODEL_CHECK)


@pytest.mark.parametrize("seed,cfg", SMALL, ids=[f"{seed}-{cfg.name}" for seed, cfg in SMALL])
def test_the_model_agrees_with_a_numpy_restatement(oracle, seed, cfg):
    assert len(SMALL) == 3 and 33 in {c.dim for _, c in SMALL}
    m = ModelIndex(cfg.dim, cfg.dtype, cfg.metric, cfg.id_offset)
    rng = np.random.default_rng(seed)
    checked = {}
    for step, op in enumerate(plan_of(seed, cfg)):
        if op.kind == "reject":
            if op.a["what"] == "add_nan":
                with pytest.raises(Exception):
                    m.add(op.a["rows"])
            continue
        if not S.is_check(op):
            S.apply_mutation(m, op)
            assert np.array_equal(bits(m.prepared()), bits(O.numpy_prepare(m.rows, {"f32": 0, "bf16": 1}[m.dtype], m.prep))), f"step {step}: prepared rows"
            continue
        assert m.count <= 2000
        want = S.expected(m, op)
        what = f"seed {seed} step {step} {op}"
        if op.kind == "pipelined":
            ops = [S.Op("search", dict(rq=rq, k=op.a["k"])) for rq in op.a["rq"][:2]]
            pairs = list(zip(want[:2], (numpy_expected(m, o) for o in ops)))
        elif op.kind == "knn_graph":            # 48 of its rows, deleted ones among them
            rows = np.sort(rng.choice(m.count, 48, replace=False))
            live = rows[~m.deleted[rows]]
            by = S.Op("search_by_ids", dict(ids=live.astype(np.uint64) + np.uint64(m.offset), k=op.a["k"], exclude_self=True))
            dead = rows[m.deleted[rows]]
            assert (want[0][dead] == ID_NONE).all() and np.isnan(want[1][dead]).all(), what
            pairs = [((want[0][live], want[1][live]), numpy_expected(m, by))]
        else:
            pairs = [(want, numpy_expected(m, op))]
        for w, g in pairs:
            for x, y in zip(w, g):
                x, y = np.asarray(x), np.asarray(y)
                assert x.shape == y.shape, what
                if x.dtype == np.float32:
                    assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(bits(x)[~np.isnan(x)], bits(y)[~np.isnan(y)]), what
                else:
                    assert np.array_equal(x, y), what
        checked[op.kind] = checked.get(op.kind, 0) + 1
    assert set(checked) >= set(S.FORMS) - {"knn_graph", "search_by_ids"}, checked
    assert checked.get("search_by_ids", 0) + checked.get("knn_graph", 0) >= 1, checked      # (the graph is the by-id search of every row)
