"""GPU tests of the search by weighted examples (vrod_search_combined) against tests/combine_model.py.

The contract: query q is fl-summed on the device, in the caller's order and with two roundings per step, from its prepared
vector (optional) and prepared stored rows; the combined vector is a raw query to the ordinary search over the eligible
rows minus q's excluded ids.  Expected values come from the model: oracle.prepare for the rows and the vector, a numpy
float32 loop for the combination (tests/test_combine_model.py shows that a reordered or fused combination changes bits at
these shapes), oracle_over for the search.  Ids and score bits are compared with support.assert_same.

Shapes: 3000 rows, d = 72 (a row stride with padding) and 128, every dtype and metric; batches of 1, 16 and 80 queries
(the stream, skinny and tiled scans); the width test runs 600 rows at d = 1 .. 4100.
"""
import ctypes as C

import numpy as np
import pytest

import combine_model as M
import support
from support import DT, ID_NONE, PATH_AUTO, THREADS, va, O, bits, eligible_rows, prep_of  # noqa: F401

pytestmark = pytest.mark.gpu

N, K = 3000, 10
SENT_ID, SENT_SC = np.uint64(0x5A5A5A5A5A5A5A5A), np.float32(-12345.5)
SENT32 = 0x5A5A5A5A


def assert_same(got, want, what=""):
    support.assert_same(*got, *want, what)


def raw_corpus(n, d, metric, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, d)).astype(np.float32)
    if metric == "ip":   # norms spread over e^2: a row is often not its own best match
        raw *= np.exp(rng.uniform(-1.0, 1.0, (n, 1))).astype(np.float32)
    return raw


def prepare(O, raw, dtype, metric):
    return O.prepare(raw, DT[dtype], prep_of(metric), threads=THREADS)


_CACHE = {}


def corpus(O, d, dtype, metric, n=N):
    """(raw rows, prepared rows) of one (shape, dtype, metric): computed once, shared, never written to."""
    key = (n, d, dtype, metric)
    if key not in _CACHE:
        raw = raw_corpus(n, d, metric, 3000 + d)
        pc = prepare(O, raw, dtype, metric)
        raw.setflags(write=False)
        pc.setflags(write=False)
        _CACHE[key] = (raw, pc)
    return _CACHE[key]


def make_index(va, raw, dtype, metric, id_offset=0):
    ix = va.Index(raw.shape[1], dtype, metric)
    ix.add(raw)
    if id_offset:
        ix.set_id_offset(id_offset)
    return ix


def random_queries(rng, nq, n, d, with_vectors, max_terms=5, rows=None):
    """1 .. max_terms terms per query, weights in [-1, 1] with both signs among them."""
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = []
    for q in range(nq):
        nt = int(rng.integers(1, max_terms + 1))
        w = rng.uniform(-1.0, 1.0, nt).astype(np.float32)
        if nt > 1:
            w[0], w[1] = abs(w[0]), -abs(w[1])
        Q = {"terms": rng.choice(rows, nt).tolist(), "weights": w.tolist()}
        if with_vectors:
            Q["vector"] = rng.standard_normal(d).astype(np.float32)
            Q["vw"] = float(rng.uniform(-1.5, 1.5))
        out.append(Q)
    return out


def call(ix, queries, k, exclude_terms=False, id_offset=0, vw=True):
    """The host form through the Python wrapper, flat arrays."""
    vec, vws, tl, tid, tw, xl, xid = M.flat(queries)
    return ix.search_combined(k, tid + np.uint64(id_offset), tw, term_lims=tl, vectors=vec, vector_weights=vws if vw else None,
                              exclude_ids=xid if xid.size else None, exclude_lims=xl if xid.size else None, exclude_terms=exclude_terms)


def raw_call(ix, queries, k, flags=0, id_offset=0, nq=None, tl=None, xl=None, with_excl=None):
    """The host form through ctypes, outputs preset to sentinels -> (rc, ids, scores)."""
    vec, vws, tl0, tid, tw, xl0, xid = M.flat(queries)
    tl = tl0 if tl is None else np.asarray(tl, np.uint32)
    xl = xl0 if xl is None else np.asarray(xl, np.uint32)
    nq = len(queries) if nq is None else nq
    tid = tid + np.uint64(id_offset)
    with_excl = bool(xid.size) if with_excl is None else with_excl
    oi = np.full((nq, k), SENT_ID, np.uint64)
    sc = np.full((nq, k), SENT_SC, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    rc = ix._L.vrod_search_combined(ix._h, p(vec), p(vws), p(tl), p(tid), p(tw), p(xl) if with_excl else None, p(xid) if with_excl else None,
                                    nq, k, flags, p(oi), p(sc))
    return rc, oi, sc


def untouched(oi, sc):
    return (oi == SENT_ID).all() and (sc == SENT_SC).all()


def device_call(va, ix, queries, k, exclude_terms=False, id_offset=0, stream=None, expect_code=None):
    """The device form: every input made on `stream` just before the call -> (ids uint64, scores) as numpy, or the outputs
    after a refused call (expect_code)."""
    import torch
    dev = torch.device("cuda:0")
    vec, vws, tl, tid, tw, xl, xid = M.flat(queries)
    stream = stream or torch.cuda.Stream(device=dev)
    nq = len(queries)
    with torch.cuda.stream(stream):
        t = lambda a, dt: None if a is None else torch.from_numpy(a.astype(dt)).to(dev, non_blocking=True)   # noqa: E731
        d_tid = t((tid + np.uint64(id_offset)).view(np.int64), np.int64)
        d_xid = t(xid.view(np.int64), np.int64) if xid.size else None
        oi = torch.full((nq, k), SENT32, dtype=torch.int64, device=dev)
        osc = torch.full((nq, k), float(SENT_SC), dtype=torch.float32, device=dev)
        args = dict(d_vectors=t(vec, np.float32), d_vector_weights=t(vws, np.float32), d_exclude_lims=t(xl.view(np.int32), np.int32) if xid.size else None,
                    d_exclude_ids=d_xid, exclude_terms=exclude_terms, out_ids=oi, out_scores=osc)
        if expect_code is None:
            ix.search_combined_device(k, t(tl.view(np.int32), np.int32), d_tid, t(tw, np.float32), **args)
        else:
            with pytest.raises(va.VrodError) as e:
                ix.search_combined_device(k, t(tl.view(np.int32), np.int32), d_tid, t(tw, np.float32), **args)
            assert e.value.code == expect_code
    return oi.cpu().numpy().view(np.uint64), osc.cpu().numpy()


# ------------------------------------------------------------------ 1. every route, dtype, metric and row stride
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [72, 128])
def test_routes_match_the_model(va, O, d, dtype, metric):
    raw, pc = corpus(O, d, dtype, metric)
    rng = np.random.default_rng(7)
    elig = np.arange(N)
    with make_index(va, raw, dtype, metric) as ix:
        for nq in (1, 16, 80):
            for with_vectors in (False, True):   # half of the batches carry a vector per query
                qs = random_queries(rng, nq, N, d, with_vectors)
                got = call(ix, qs, K, vw=nq != 16)   # (nq = 16 with vectors: the weights pointer is NULL, every weight 1)
                if with_vectors and nq == 16:
                    for Q in qs:
                        Q["vw"] = None
                st = ix.last_stats()
                assert_same(got, M.search(O, raw, pc, dtype, metric, qs, K, elig), f"nq {nq} vectors {with_vectors}")
                assert st["k"] == K and st["nq"] == nq, st


# ------------------------------------------------------------------ 2. order
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2")])
def test_order_of_the_terms_is_honoured(va, O, dtype, metric):
    """The same terms in two orders: each result equals its own model result.  (That the two combined vectors differ in
    bits, so that a kernel which sorted or reassociated the terms would fail here, is asserted on the model.)"""
    d = 72
    raw, pc = corpus(O, d, dtype, metric)
    rng = np.random.default_rng(13)
    fwd, rev, differ = [], [], 0
    for q in range(24):
        terms = rng.choice(N, 5, replace=False).tolist()
        w = rng.uniform(-1.0, 1.0, 5).astype(np.float32).tolist()
        fwd.append({"terms": terms, "weights": w})
        rev.append({"terms": terms[::-1], "weights": w[::-1]})
        a = M.combine(O, pc, dtype, metric, None, None, terms, w)
        b = M.combine(O, pc, dtype, metric, None, None, terms[::-1], w[::-1])
        differ += not np.array_equal(bits(a), bits(b))
    assert differ >= 12
    with make_index(va, raw, dtype, metric) as ix:
        assert_same(call(ix, fwd, K), M.search(O, raw, pc, dtype, metric, fwd, K, np.arange(N)), "forward")
        assert_same(call(ix, rev, K), M.search(O, raw, pc, dtype, metric, rev, K, np.arange(N)), "reversed")


# ------------------------------------------------------------------ 3. exact cancellation
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_exact_cancellation_is_the_zero_norm_query(va, O, dtype):
    raw, pc = corpus(O, 72, dtype, "cosine")
    qs = [{"terms": [r, r], "weights": [1.0, -1.0]} for r in (0, 17, 2999)] + [{"terms": [5, 9, 5, 9], "weights": [0.5, -2.0, -0.5, 2.0]}]
    assert all(not M.combine(O, pc, dtype, "cosine", None, None, Q["terms"], Q["weights"]).any() for Q in qs[:3])
    want = M.search(O, raw, pc, dtype, "cosine", qs, K, np.arange(N))
    zero = support.oracle_over(O, raw, np.zeros((1, 72), np.float32), K, dtype, "cosine", np.arange(N))
    for q in range(3):
        assert_same((want[0][q], want[1][q]), (zero[0][0], zero[1][0]), "the model's own premise")
    with make_index(va, raw, dtype, "cosine") as ix:
        assert_same(call(ix, qs, K), want, "cancellation")


# ------------------------------------------------------------------ 4. cross-check with vrod_search_by_ids
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_term_of_weight_one_is_search_by_ids(va, O, dtype, metric):
    """L2 and IP handles prepare a query by (at most) rounding it to bf16, which a stored row already is: one term of
    weight 1 is the stored row again, and the two entry points must agree bit for bit, with and without the self drop."""
    raw, pc = corpus(O, 72, dtype, metric)
    rows = np.random.default_rng(3).choice(N, 40, replace=False)
    qs = [{"terms": [int(r)], "weights": [1.0]} for r in rows]
    with make_index(va, raw, dtype, metric) as ix:
        for ex in (False, True):
            got = call(ix, qs, K, exclude_terms=ex)
            assert_same(got, ix.search_by_ids(rows, K, exclude_self=ex), f"exclude {ex}")
            assert_same(got, M.search(O, raw, pc, dtype, metric, qs, K, np.arange(N), exclude_terms=ex), f"model, exclude {ex}")
            if ex:
                assert not (got[0] == rows[:, None].astype(np.uint64)).any()


# ------------------------------------------------------------------ 5. exclusion
def test_exclusion_by_terms_and_by_list(va, O):
    dtype, metric, d, off = "bf16", "cosine", 72, 10 ** 9
    raw, pc = corpus(O, d, dtype, metric)
    rng = np.random.default_rng(17)
    dead = rng.choice(N, 200, replace=False)
    elig = eligible_rows(N, deleted=dead)
    with make_index(va, raw, dtype, metric, id_offset=off) as ix:
        ix.delete(dead + off)
        qs = random_queries(rng, 20, N, d, False, rows=elig)
        plain = M.search(O, raw, pc, dtype, metric, qs, 40, elig, id_offset=off)
        # the terms flag alone: several terms per query, each of them gone from its own result only
        got = call(ix, qs, K, exclude_terms=True, id_offset=off)
        assert_same(got, M.search(O, raw, pc, dtype, metric, qs, K, elig, exclude_terms=True, id_offset=off), "terms flag")
        for q, Q in enumerate(qs):
            assert not np.isin(got[0][q], np.array(Q["terms"], np.uint64) + np.uint64(off)).any()
        # a list of ids as a seen-list really looks: some of the query's own best rows, repeated; deleted rows; ids past
        # the rows and below the offset; VROD_ID_NONE.  Only the first kind changes anything.
        for q, Q in enumerate(qs):
            seen = plain[0][q][[0, 2, 2, 5, 0]].tolist()
            Q["exclude"] = seen + [int(dead[q]) + off, int(dead[q]) + off, off + N, off + N + 12345, off - 1, 5, int(ID_NONE)]
        want = M.search(O, raw, pc, dtype, metric, qs, K, elig, id_offset=off)
        assert_same(call(ix, qs, K, id_offset=off), want, "exclude list")
        for q in range(len(qs)):
            assert want[0][q].tolist() == [i for i in plain[0][q].tolist() if i not in plain[0][q][[0, 2, 5]].tolist()][:K]
        # ... and both together
        assert_same(call(ix, qs, K, exclude_terms=True, id_offset=off),
                    M.search(O, raw, pc, dtype, metric, qs, K, elig, exclude_terms=True, id_offset=off), "list and terms")
        # only one query of the batch excludes anything: the others' rows are the unexcluded search's
        for Q in qs:
            Q.pop("exclude")
        qs[7]["exclude"] = plain[0][7][:3].tolist()
        got = call(ix, qs, K, id_offset=off)
        assert_same(got, M.search(O, raw, pc, dtype, metric, qs, K, elig, id_offset=off), "one query excludes")
        others = [q for q in range(len(qs)) if q != 7]
        assert_same((got[0][others], got[1][others]), (plain[0][others, :K], plain[1][others, :K]), "the queries that exclude nothing")
        assert got[0][7].tolist() == plain[0][7][3:3 + K].tolist()


@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "ip")])
def test_drops_on_both_sides_of_the_chunk_boundaries(va, O, dtype, metric):
    """k = 200.  Query A excludes 300 ids, query B 330, so the search runs with k1 = 530 and the drop launch walks lists of
    530 positions in chunks of 256.  The excluded ids are taken from the model's unexcluded ranking, so their list
    positions are known: both queries drop entries at 254 .. 257 and at 510 .. 513, and B drops 322 of its first 512
    entries, so that its walk must go on into the third chunk for its last survivors."""
    k, d = 200, 72
    raw, pc = corpus(O, d, dtype, metric)
    qs = [{"terms": [11, 222], "weights": [1.0, 0.5]}, {"terms": [1500], "weights": [-1.0]}]
    rank, _ = M.search(O, raw, pc, dtype, metric, qs, 800, np.arange(N))
    pos_a = np.r_[100:200, 250:262, 400:450, 505:519, 600:724]
    pos_b = np.r_[0:150, 200:260, 300:400, 500:520]
    assert pos_a.size == 300 and pos_b.size == 330 and (pos_b < 512).sum() == 322
    qs[0]["exclude"] = rank[0][pos_a].tolist()
    qs[1]["exclude"] = rank[1][pos_b].tolist()
    want = M.search(O, raw, pc, dtype, metric, qs, k, np.arange(N))
    assert want[0][0].tolist() == np.delete(rank[0], pos_a)[:k].tolist() and want[0][1].tolist() == np.delete(rank[1], pos_b)[:k].tolist()
    assert want[0][1][-1] == rank[1][529]   # B's last survivor sits at list position 529
    with make_index(va, raw, dtype, metric) as ix:
        assert_same(call(ix, qs, k), want, "300 / 330 excluded")
        assert ix.last_stats()["k"] == k


def test_excluded_set_that_leaves_three_rows(va, O):
    dtype, metric, d = "f32", "l2", 72
    raw, pc = corpus(O, d, dtype, metric)
    allow = np.zeros(N, bool)
    allow[::6] = True                                   # 500 eligible rows
    elig = np.flatnonzero(allow)
    keep = elig[[3, 250, 499]]
    with make_index(va, raw, dtype, metric) as ix:
        ix.set_filter(allow)
        qs = [{"terms": [7], "weights": [1.0], "exclude": np.setdiff1d(elig, keep).tolist()},
              {"terms": [8, 9], "weights": [1.0, 1.0]}]
        got = call(ix, qs, K)
        assert_same(got, M.search(O, raw, pc, dtype, metric, qs, K, elig), "all but three")
        assert sorted(got[0][0][:3].tolist()) == keep.tolist() and (got[0][0][3:] == ID_NONE).all() and np.isnan(got[1][0][3:]).all()
        assert (got[0][1] != ID_NONE).all()


# ------------------------------------------------------------------ 6. handle state
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2")])
def test_after_delete_update_filter_offset_and_compact(va, O, dtype, metric):
    d = 72
    base, _ = corpus(O, d, dtype, metric)
    raw = base.copy()
    rng = np.random.default_rng(21)
    live = np.ones(N, bool)

    def check(ix, what, off=0, allow=None, rows=raw):
        pc = prepare(O, rows, dtype, metric)
        ok = live[:rows.shape[0]] if rows is raw else np.ones(rows.shape[0], bool)
        elig = np.flatnonzero(ok & (allow if allow is not None else True))
        qs = random_queries(rng, 12, rows.shape[0], d, True, rows=np.flatnonzero(ok))
        for q in (0, 5):
            qs[q]["exclude"] = [int(x) + off for x in rng.choice(elig, 4)]
        for ex in (False, True):
            assert_same(call(ix, qs, K, exclude_terms=ex, id_offset=off),
                        M.search(O, rows, pc, dtype, metric, qs, K, elig, exclude_terms=ex, id_offset=off), f"{what}, exclude terms {ex}")
        return qs

    with make_index(va, raw, dtype, metric) as ix:
        dead = rng.choice(N, N // 10, replace=False)
        ix.delete(dead)
        live[dead] = False
        check(ix, "deleted")
        # a term naming a deleted row, or a row past the count: the whole call fails, nothing is written -- both forms
        good = int(np.flatnonzero(live)[0])
        for bad in (int(dead[0]), N, 1 << 40):
            qs = [{"terms": [good], "weights": [1.0]}, {"terms": [good, bad], "weights": [1.0, 1.0]}]
            for flags in (0, 1):
                rc, oi, sc = raw_call(ix, qs, K, flags)
                assert rc == 1 and untouched(oi, sc), (bad, flags)
            oi, sc = device_call(va, ix, qs, K, expect_code=1)
            assert (oi == SENT32).all() and (sc == SENT_SC).all(), bad
        upd = rng.choice(np.flatnonzero(live), 50, replace=False)
        raw[upd] = raw_corpus(50, d, metric, 77)
        ix.update(upd, raw[upd])
        check(ix, "updated")
        upd_q = [{"terms": [int(upd[0]), int(upd[1])], "weights": [1.0, -0.25]}]
        assert_same(call(ix, upd_q, K), M.search(O, raw, prepare(O, raw, dtype, metric), dtype, metric, upd_q, K, np.flatnonzero(live)), "updated rows as terms")
        allow = rng.random(N) < 0.4
        ix.set_filter(allow)
        check(ix, "filtered", allow=allow)
        ix.set_filter(None)
        ix.set_id_offset(5000)
        check(ix, "offset", off=5000)
        rc, oi, sc = raw_call(ix, [{"terms": [good], "weights": [1.0]}], K)   # the id without the offset names no row (good < 5000)
        assert rc == 1 and untouched(oi, sc)
        new_ids = ix.compact()
        assert ix.count == live.sum()
        raw2 = np.ascontiguousarray(raw[live])
        check(ix, "compacted", off=5000, rows=raw2)
        rc, oi, sc = raw_call(ix, [{"terms": [int(live.sum())], "weights": [1.0]}], K, id_offset=5000)
        assert rc == 1 and untouched(oi, sc)
        assert (new_ids[np.flatnonzero(live)] != ID_NONE).all()


# ------------------------------------------------------------------ 7. device form
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "ip")])
def test_device_form_matches_the_host_form(va, O, dtype, metric):
    import torch
    d = 72
    raw, pc = corpus(O, d, dtype, metric)
    rng = np.random.default_rng(5)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    with make_index(va, raw, dtype, metric) as ix:
        ix.delete([11])
        elig = eligible_rows(N, deleted=[11])
        for with_vectors in (False, True):
            qs = random_queries(rng, 40, N, d, with_vectors, rows=elig)
            plain = M.search(O, raw, pc, dtype, metric, qs, K, elig)
            for q in range(0, 40, 3):
                qs[q]["exclude"] = plain[0][q][:4].tolist() + [11, int(ID_NONE)]
            for ex in (False, True):
                host = call(ix, qs, K, exclude_terms=ex)
                got = device_call(va, ix, qs, K, exclude_terms=ex, stream=stream)
                assert_same(got, host, f"device form, vectors {with_vectors}, exclude terms {ex}")
                assert_same(got, M.search(O, raw, pc, dtype, metric, qs, K, elig, exclude_terms=ex), "device form against the model")
        # nothing excluded: the search writes the caller's tensors directly
        qs = random_queries(rng, 5, N, d, False, rows=elig)
        assert_same(device_call(va, ix, qs, K, stream=stream), M.search(O, raw, pc, dtype, metric, qs, K, elig), "device form, no exclusion")


# ------------------------------------------------------------------ 8. widths
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [1, 3, 33, 65, 257, 1100, 4100])
def test_widths(va, O, d, dtype):
    """Row widths around the 16-B unit and its scalar tail, below and above the switch from a wave to a work-group per
    query (1024 fp32 / 2048 bf16 values), with one query of 256 terms per width."""
    n, metric = 600, "cosine" if dtype == "bf16" else "ip"
    raw, pc = corpus(O, d, dtype, metric, n=n)
    rng = np.random.default_rng(100 + d)
    with make_index(va, raw, dtype, metric) as ix:
        qs = random_queries(rng, 6, n, d, True)
        qs.append({"terms": rng.integers(0, n, 256).tolist(), "weights": rng.uniform(-1, 1, 256).astype(np.float32).tolist(),
                   "vector": rng.standard_normal(d).astype(np.float32), "vw": 0.75})
        assert_same(call(ix, qs, K), M.search(O, raw, pc, dtype, metric, qs, K, np.arange(n)), f"d {d}")
        no_vec = [{"terms": Q["terms"], "weights": Q["weights"], "exclude": Q["terms"][:2]} for Q in qs]
        assert_same(call(ix, no_vec, K, exclude_terms=True), M.search(O, raw, pc, dtype, metric, no_vec, K, np.arange(n), exclude_terms=True),
                    f"d {d}, terms only")


# ------------------------------------------------------------------ 9. overflow, NaN and Inf
def test_overflow_and_non_finite_inputs(va, O):
    d = 72
    raw, pc = corpus(O, d, "f32", "ip")
    big = np.flatnonzero((np.abs(pc) > 1.0).any(axis=1))[:2].tolist()
    assert len(big) == 2
    ok = {"terms": [1, 2], "weights": [1.0, 1.0]}
    vec = raw[5].copy()
    with make_index(va, raw, "f32", "ip") as ix:
        cases = {
            "overflow": [ok, {"terms": big, "weights": [3e38, 3e38]}],
            "NaN weight": [ok, {"terms": [3], "weights": [float("nan")]}],
            "Inf weight": [{"terms": [3, 4], "weights": [1.0, float("-inf")]}, ok],
            "NaN vector weight": [dict(ok, vector=vec, vw=1.0), dict(ok, vector=vec, vw=float("nan"))],
            "Inf vector weight": [dict(ok, vector=vec, vw=float("inf")), dict(ok, vector=vec, vw=1.0)],
            "NaN vector": [dict(ok, vector=vec, vw=1.0), dict(ok, vector=np.where(np.arange(d) == 70, np.nan, vec).astype(np.float32), vw=1.0)],
            "Inf vector": [dict(ok, vector=np.where(np.arange(d) == 0, np.inf, vec).astype(np.float32), vw=1.0), dict(ok, vector=vec, vw=1.0)],
        }
        for what, qs in cases.items():
            for flags in (0, 1):
                rc, oi, sc = raw_call(ix, qs, K, flags)
                assert rc == 2 and untouched(oi, sc), (what, flags)
            oi, sc = device_call(va, ix, qs, K, expect_code=2)
            assert (oi == SENT32).all() and (sc == SENT_SC).all(), what
        # a sum that overflows only in between is an overflow too (the contract is per step); one that stays finite is not
        rc, oi, sc = raw_call(ix, [{"terms": big + big, "weights": [3e38, 3e38, -3e38, -3e38]}], K)
        assert rc == 2 and untouched(oi, sc)
        fine = [{"terms": big, "weights": [1e15, -1e15]}, ok]
        assert_same(call(ix, fine, K), M.search(O, raw, pc, "f32", "ip", fine, K, np.arange(N)), "large but finite")
        assert ix.pending == 0


# ------------------------------------------------------------------ 10. refusals on a live handle
def test_refusals_on_a_live_handle(va, O):
    raw, pc = corpus(O, 72, "bf16", "cosine")
    ok = {"terms": [1, 2], "weights": [1.0, -1.0]}
    vec = raw[9].copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    with make_index(va, raw, "bf16", "cosine") as ix:
        L, h = ix._L, ix._h

        def refused(rc_oi_sc, what, code=1):
            rc, oi, sc = rc_oi_sc
            assert rc == code and untouched(oi, sc), what

        # lims that do not start at 0, that decrease; the same for the exclude lims
        refused(raw_call(ix, [ok, ok], K, tl=[1, 2, 4]), "term_lims[0] != 0")
        refused(raw_call(ix, [ok, ok], K, tl=[0, 3, 2]), "term_lims decreases")
        ex = [dict(ok, exclude=[5, 6]), dict(ok, exclude=[7])]
        refused(raw_call(ix, ex, K, xl=[1, 2, 3]), "exclude_lims[0] != 0")
        refused(raw_call(ix, ex, K, xl=[0, 3, 2]), "exclude_lims decreases")
        # a query without an operand; with a vector it has one
        refused(raw_call(ix, [ok, {"terms": [], "weights": []}], K), "no operand")
        alone = [dict(ok, vector=vec), {"terms": [], "weights": [], "vector": vec}]
        assert_same(call(ix, alone, K), M.search(O, raw, pc, "bf16", "cosine", alone, K, np.arange(N)), "a vector alone is an operand")
        # 256 terms pass, 257 do not; 1024 excluded entries pass, 1025 do not, the terms counted under the flag
        t256 = {"terms": list(range(256)), "weights": [0.01] * 256}
        t257 = {"terms": list(range(257)), "weights": [0.01] * 257}
        assert_same(call(ix, [t256], K), M.search(O, raw, pc, "bf16", "cosine", [t256], K, np.arange(N)), "256 terms")
        refused(raw_call(ix, [ok, t257], K), "257 terms")
        x1024 = dict(ok, exclude=list(range(1000, 2024)))
        assert_same(call(ix, [x1024], K), M.search(O, raw, pc, "bf16", "cosine", [x1024], K, np.arange(N)), "1024 excluded")
        refused(raw_call(ix, [dict(ok, exclude=list(range(1000, 2025)))], K), "1025 excluded")
        x1022 = dict(ok, exclude=list(range(1000, 2022)))
        assert_same(call(ix, [x1022], K, exclude_terms=True), M.search(O, raw, pc, "bf16", "cosine", [x1022], K, np.arange(N), exclude_terms=True),
                    "1022 listed + 2 terms")
        refused(raw_call(ix, [dict(ok, exclude=list(range(1000, 2023)))], K, flags=1), "1023 listed + 2 terms")
        # flag bits, k = 0, k past VROD_MAX_K, k + the largest excluded count past it
        for flags in (2, 0x80000001, 0xFFFFFFFE):
            refused(raw_call(ix, [ok], K, flags), f"flags {flags:#x}")
        refused(raw_call(ix, [ok], 0), "k = 0")
        refused(raw_call(ix, [ok], va.MAX_K + 1), "k > MAX_K")
        refused(raw_call(ix, [ok], va.MAX_K, 1), "k + 2 terms > MAX_K")
        refused(raw_call(ix, [ok, dict(ok, exclude=[5])], va.MAX_K), "k + 1 excluded > MAX_K")
        x3 = [ok, dict(ok, exclude=[5, 6, 7])]
        assert_same(call(ix, x3, va.MAX_K - 3), M.search(O, raw, pc, "bf16", "cosine", x3, va.MAX_K - 3, np.arange(N)), "k + 3 = MAX_K")
        # null required pointers
        _, _, tl, tid, tw, _, _ = M.flat([ok])
        oi = np.full((1, K), SENT_ID, np.uint64)
        sc = np.full((1, K), SENT_SC, np.float32)
        xl = np.array([0, 1], np.uint32)
        for args in ((None, p(tid), p(tw), None, None, p(oi), p(sc)), (p(tl), None, p(tw), None, None, p(oi), p(sc)),
                     (p(tl), p(tid), None, None, None, p(oi), p(sc)), (p(tl), p(tid), p(tw), p(xl), None, p(oi), p(sc)),
                     (p(tl), p(tid), p(tw), None, None, None, p(sc)), (p(tl), p(tid), p(tw), None, None, p(oi), None)):
            assert L.vrod_search_combined(h, None, None, *args[:5], 1, K, 0, *args[5:]) == 1
            assert untouched(oi, sc)
        # nq == 0 is fine and writes nothing
        assert L.vrod_search_combined(h, None, None, None, None, None, None, None, 0, K, 0, None, None) == 0
        # the handle is as usable as before
        assert_same(call(ix, [ok], K), M.search(O, raw, pc, "bf16", "cosine", [ok], K, np.arange(N)), "after the refusals")


def test_empty_handle_and_no_eligible_row(va, O):
    raw, _ = corpus(O, 72, "bf16", "cosine")
    vec = raw[:2].copy()
    with va.Index(72, "bf16", "cosine") as ix:
        got = ix.search_combined(K, [], [], term_lims=[0, 0, 0], vectors=vec)
        assert (got[0] == ID_NONE).all() and np.isnan(got[1]).all()
        rc, oi, sc = raw_call(ix, [{"terms": [0], "weights": [1.0]}], K)   # no row is live on an empty handle
        assert rc == 1 and untouched(oi, sc)
    with make_index(va, raw, "bf16", "cosine") as ix:
        ix.set_filter(np.zeros(N, bool))
        got = call(ix, [{"terms": [1, 2], "weights": [1.0, 1.0], "exclude": [3]}], K, exclude_terms=True)
        assert (got[0] == ID_NONE).all() and np.isnan(got[1]).all()


def test_pending_search_blocks_both_forms(va, O):
    import torch
    raw, pc = corpus(O, 72, "bf16", "cosine")
    dev = torch.device("cuda:0")
    ok = {"terms": [1, 2], "weights": [1.0, 0.5]}
    with make_index(va, raw, "bf16", "cosine") as ix:
        dq = torch.from_numpy(raw[:4].copy()).to(dev)
        oi = torch.empty((4, K), dtype=torch.int64, device=dev)
        osc = torch.empty((4, K), dtype=torch.float32, device=dev)
        ix.search_begin_device(dq, K, oi, osc)
        assert ix.pending == 1
        rc, hi, hs = raw_call(ix, [ok], K, 1)
        assert rc == 1 and untouched(hi, hs)
        di, ds = device_call(va, ix, [ok], K, expect_code=1)
        assert (di == SENT32).all() and (ds == SENT_SC).all()
        assert ix.pending == 1
        ix.search_end()
        assert_same(call(ix, [ok], K, exclude_terms=True), M.search(O, raw, pc, "bf16", "cosine", [ok], K, np.arange(N), exclude_terms=True),
                    "after the pending search")


def test_multi_device_handle_is_unsupported(va, O):
    raw, _ = corpus(O, 72, "bf16", "cosine")
    ok = {"terms": [1, 2], "weights": [1.0, 0.5]}
    with va.Index(72, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        rc, hi, hs = raw_call(ix, [ok], K)
        assert rc == 6 and untouched(hi, hs)
        di, ds = device_call(va, ix, [ok], K, expect_code=6)
        assert (di == SENT32).all() and (ds == SENT_SC).all()
