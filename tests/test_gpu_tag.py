"""GPU tests of row tags and the tagged search (vrod_index_set_tags / vrod_search_tagged) against the CPU oracle.

The contract: query q of a tagged search gets, bit for bit, what the oracle returns over the rows that are live, allowed
and match preds[q] -- tag_model.TagModelIndex: scan_topk(prepared[those rows], ...), ids mapped back.  The rows are taken
in ascending order, so ties still break by the smaller id; slots beyond them are (ID_NONE, NaN).

One corpus of 40 003 rows (the last 64-row wave, the last 32-bit mask word and the last count block are all partial;
d = 64, and d = 100 whose tail chunk has padding that must not be walked).  Its tags:
  bit 0   on half of the rows (AUTO scans it densely), bit 63 on a tenth -- a 32-bit slip loses one of them;
  bits 2, 3, 4, 5 on exactly 63, 64, 65 and 8 193 (= kSelectChunk + 1) rows; bit 1 on ONE row besides the all-ones rows
          (the predicate {any: bit 1, none: bit 6} sees exactly that row);
  200 pairs of the bits 8 .. 28 on 12 - 28 rows each, drawn from the whole corpus: they overlap each other and the rest;
  3 rows carry all 64 bits (they alone carry bits 6 and 7) and sit in every list at once; what is left carries 0.
"""
import itertools
import os
import re

import numpy as np
import pytest

from tag_model import TagModelIndex, distinct_preds, tag_matches
from support import (  # noqa: F401
    PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, ID_NONE, va, assert_same, row_bytes, takes_segments)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 40_003
ALL_ONES = 0xFFFFFFFFFFFFFFFF
N_ONES = 3


def B(*bits_):
    return sum(1 << b for b in bits_)


B_HALF, B_TENTH, B_ONE, B_ONLY_ONES, B_ONLY_ONES2 = 0, 63, 1, 6, 7
B_EXACT = {2: 63, 3: 64, 4: 65, 5: 8193}            # bit -> rows that carry it (the all-ones rows among them)
PAIRS = list(itertools.combinations(range(8, 29), 2))[:200]

P_HALF = (B(B_HALF), 0, 0)
P_TENTH = (B(B_TENTH), 0, 0)
P_THREE = (B(2, 3, 4), 0, 0)                         # a union of three bits
P_ONE_ROW = (B(B_ONE), 0, B(B_ONLY_ONES))            # any + none: exactly one row
P_EVERY = (0, 0, 0)
P_NO_ROW = (0, B(B_ONLY_ONES2), B(B_ONLY_ONES))      # satisfiable, but only the all-ones rows carry bit 7, and they carry bit 6
P_UNSAT = (B(B_HALF), B(9), B(9, 40))                # all & none != 0
P_UNSAT2 = (0, ALL_ONES, 1 << 63)


def p_pair(j):
    return (0, B(*PAIRS[j]), 0)                      # all of two bits


def make_tags(rng):
    tags = np.zeros(N, np.uint64)
    perm = rng.permutation(N)
    ones = perm[:N_ONES]

    def put(rows, mask):
        tags[rows] |= np.uint64(mask)
    put(perm[N_ONES:N_ONES + N // 2], B(B_HALF))
    put(rng.choice(perm[N_ONES:], N // 10, replace=False), B(B_TENTH))
    put(rng.choice(perm[N_ONES:], 1), B(B_ONE))
    for b, n in B_EXACT.items():
        put(rng.choice(perm[N_ONES:], n - N_ONES, replace=False), B(b))
    for (a, b), n in zip(PAIRS, rng.integers(12, 29, len(PAIRS))):
        put(rng.choice(perm[N_ONES:], int(n), replace=False), B(a, b))
    tags[ones] = np.uint64(ALL_ONES)
    return tags


def batch_preds(rng, nq):
    if nq == 1:
        q = [P_TENTH]
    elif nq == 9:
        q = [P_HALF, P_THREE, p_pair(0), P_ONE_ROW, P_EVERY, P_NO_ROW, P_UNSAT, p_pair(0), P_TENTH]
    else:
        q = [P_HALF] * 256 + [P_THREE] * 9 + [P_TENTH] * 3 + [P_ONE_ROW, P_EVERY, P_EVERY, P_NO_ROW, P_UNSAT, P_UNSAT2, P_UNSAT]
        q += [(B(b), 0, 0) for b in B_EXACT] + [(B(5), 0, B(B_HALF)), (B(B_TENTH), B(B_HALF), B(5))]
        q += [p_pair(int(j)) for j in rng.integers(0, len(PAIRS), nq - len(q))]
        q = [q[i] for i in rng.permutation(len(q))]
    assert len(q) == nq
    return np.array(q, np.uint64)


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20263)
    tags = make_tags(rng)
    corpora = {d: rng.standard_normal((N, d)).astype(np.float32) for d in (64, 100)}
    queries = {d: rng.standard_normal((300, d)).astype(np.float32) for d in (64, 100)}
    preds = {nq: batch_preds(rng, nq) for nq in (1, 9, 300)}
    assert_corpus(tags, preds)
    return tags, corpora, queries, preds


def assert_corpus(tags, preds):
    """The tag layout the tests' cases rest on."""
    count = lambda p: int(tag_matches(tags, p).sum())
    assert count((ALL_ONES, ALL_ONES, 0)) == N_ONES
    assert count(P_HALF) == N // 2 + N_ONES and count(P_TENTH) == N // 10 + N_ONES
    for b, n in B_EXACT.items():
        assert count((B(b), 0, 0)) == n
    assert count(P_ONE_ROW) == 1 and count(P_NO_ROW) == 0 and count(P_EVERY) == N
    parts = [count((B(b), 0, 0)) for b in (2, 3, 4)]
    assert count(P_THREE) > max(parts) and count(P_THREE) <= sum(parts)           # a union larger than each part
    sizes = [count(p_pair(j)) for j in range(len(PAIRS))]
    assert min(sizes) >= 12 + N_ONES and max(sizes) < 64
    rows_of = [set(np.flatnonzero(tag_matches(tags, p_pair(j))).tolist()) for j in range(len(PAIRS))]
    assert sum(1 for a, b in itertools.combinations(rows_of, 2) if len(a & b) > N_ONES) > 10    # the lists overlap
    assert (tags == 0).sum() > N // 4
    assert len(distinct_preds(preds[300])) > 30 and (preds[300] == np.array(P_HALF, np.uint64)).all(axis=1).sum() == 256


def check_stats(st, path, dtype, dim, model, preds, k, what):
    nq, n = len(preds), model.count
    assert st["nq"] == nq and st["k"] == k, f"{what}: {st}"
    rb = row_bytes(dtype, dim)
    want_bytes = want_flops = 0.0
    any_dense = False
    for p in distinct_preds(preds):
        if p[1] & p[2]:
            continue                                                                 # unsatisfiable: in no group
        m, nqg = int(model.matching(p).size), int((preds == np.array(p, np.uint64)).all(axis=1).sum())
        if takes_segments(path, dtype, n, m, nqg, dim):
            want_bytes += m * rb
            want_flops += 2.0 * nqg * m * dim
        else:
            any_dense = True
            want_bytes += n * rb
            want_flops += 2.0 * nqg * n * dim
    assert st["scan_bytes"] == want_bytes and st["scan_flops"] == want_flops, f"{what}: {st} want {want_bytes} {want_flops}"
    if not any_dense:
        assert st["path"] == PATH_GATHER and st["kprime"] == 0, f"{what}: {st}"
        assert st["max_fast_err"] == 0 and st["eps_bound"] == 0 and st["fallback_queries"] == 0 and st["band_queries"] == 0, f"{what}: {st}"
    else:
        assert st["path"] != PATH_GATHER, f"{what}: {st}"
        if path != PATH_AUTO:
            assert st["path"] == path, f"{what}: {st}"
        if st["path"] != PATH_EXACT and np.isfinite(st["eps_bound"]):
            assert st["max_fast_err"] <= st["eps_bound"], f"{what}: {st}"
    return any_dense


# ---------------------------------------------------------------- every route x dtype x metric
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [64, 100])
def test_every_route(va, world, dim, dtype, metric):
    tags, corpora, queries, preds = world
    raw, k = corpora[dim], 10
    model = TagModelIndex(dim, dtype, metric)
    model.add(raw)
    model.set_tags(0, tags)
    want = {nq: model.search_tagged(queries[dim][:nq], k, preds[nq]) for nq in (1, 9, 300)}
    plain = model.search(queries[dim], k)
    with va.Index(dim, dtype, metric) as ix:
        ix.add(raw)
        ix.set_tags(0, tags)
        assert np.array_equal(ix.get_tags(0, N), tags)
        for path in (PATH_GATHER, PATH_MFMA, PATH_EXACT, PATH_STREAM, PATH_AUTO):
            ix.set_path(path)
            for nq in (1, 9, 300):
                what = f"{dim}/{dtype}/{metric}/path{path}/nq{nq}"
                ids, sc = ix.search_tagged(queries[dim][:nq], k, preds[nq])
                st = ix.last_stats()
                print(what, st)
                assert_same(ids, sc, *want[nq], what)
                dense = check_stats(st, path, dtype, dim, model, preds[nq], k, what)
                every = np.flatnonzero((preds[nq] == 0).all(axis=1))
                assert_same(ids[every], sc[every], plain[0][every], plain[1][every], what + " {0,0,0}")
                unsat = np.flatnonzero((preds[nq][:, 1] & preds[nq][:, 2]) != 0)
                assert (ids[unsat] == ID_NONE).all() and np.isnan(sc[unsat]).all(), what
                if path == PATH_AUTO and nq == 300:
                    assert dense and st["path"] == PATH_MFMA, f"{what}: {st}"      # the 50 % bit, 256 queries: a batched scan
            ids, sc = ix.search(queries[dim][:9], k)                                  # the plain search under the same handle
            assert_same(ids, sc, plain[0][:9], plain[1][:9], f"{dim}/{dtype}/{metric}/path{path} plain")


# ---------------------------------------------------------------- stats: sums and maxima over the scans
@pytest.mark.parametrize("path", [PATH_EXACT, PATH_STREAM])
def test_stats_are_sums_and_maxima_over_the_scans(va, path):
    """Under a forced scan path every distinct predicate takes one masked search.  The same search through the public
    interface is set_filter(the predicate's rows) + search(its queries) under the same path: the tagged search's
    counters are those searches' sums (scan_launches, fallback_queries, band_queries) and maxima (kprime, eps_bound,
    max_fast_err), its path the last one's."""
    rng = np.random.default_rng(47)
    n, dim, k = 6_001, 64, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    tags = rng.integers(0, 8, n).astype(np.uint64) | (np.uint64(1) << np.uint64(63))
    rq = rng.standard_normal((8, dim)).astype(np.float32)
    preds = np.array([(1, 0, 0), (0, 6, 0), (1, 0, 0), (0, 0, 4), (0, 6, 0), (1, 0, 0), (0, 0, 4), (0, 0, 4)], np.uint64)
    want = {"scan_launches": 0, "fallback_queries": 0, "band_queries": 0, "kprime": 0, "eps_bound": 0.0, "max_fast_err": 0.0}
    with va.Index(dim, "bf16", "cosine") as ix, va.Index(dim, "bf16", "cosine") as ref:
        ix.add(raw)
        ix.set_tags(0, tags)
        ix.set_path(path)
        ref.add(raw)
        ref.set_path(path)
        ids, sc = ix.search_tagged(rq, k, preds)
        st = ix.last_stats()
        for p in distinct_preds(preds):                                              # the order the groups run in
            qs = np.flatnonzero((preds == np.array(p, np.uint64)).all(axis=1))
            ref.set_filter(tag_matches(tags, p))
            ri, rs = ref.search(rq[qs], k)
            assert_same(ids[qs], sc[qs], ri, rs, f"path{path} {p}")
            r = ref.last_stats()
            print(path, p, r)
            for key in ("scan_launches", "fallback_queries", "band_queries"):
                want[key] += r[key]
            for key in ("kprime", "eps_bound", "max_fast_err"):
                want[key] = max(want[key], r[key])
            want["path"] = r["path"]
    print(path, st)
    assert {key: st[key] for key in want} == want, (st, want)
    assert st["path"] == path and st["fallback_queries"] + st["scan_launches"] > 0      # (EXACT counts no scan launch, as vrod_search)


# ---------------------------------------------------------------- one row in many lists
def test_a_row_sits_in_every_list_it_matches(va):
    rng = np.random.default_rng(41)
    n, dim, k = 4_099, 64, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((9, dim)).astype(np.float32)
    preds = np.array([(0, 0, 0), (1, 0, 0), (1 << 63, 0, 0), (0, ALL_ONES, 0), (0, B(0, 63), 0), (B(31, 32), 0, 0), (ALL_ONES, B(5), 0),
                      (B(17), B(40), 0), (0, B(32), 0)], np.uint64)
    assert len(distinct_preds(preds)) == 9
    for dtype, metric in (("bf16", "cosine"), ("f32", "l2")):
        with va.Index(dim, dtype, metric) as ix:
            ix.add(raw)
            ix.set_tags(0, np.full(n, ALL_ONES, np.uint64))
            plain = ix.search(rq, k)
            ix.set_path(PATH_GATHER)
            ids, sc = ix.search_tagged(rq, k, preds)
            st = ix.last_stats()
            assert_same(ids, sc, *plain, f"{dtype}/{metric}")
            assert st["path"] == PATH_GATHER and st["scan_bytes"] == 9.0 * n * row_bytes(dtype, dim), st


# ---------------------------------------------------------------- more groups than one pass
def groups_per_pass():
    text = open(os.path.join(ROOT, "vrod_amd", "csrc", "tag_plan.h")).read()
    return int(re.search(r"constexpr uint32_t kTagGroupsPerPass = (\d+);", text).group(1))


@pytest.mark.parametrize("path", [PATH_GATHER, PATH_AUTO])
def test_more_groups_than_one_pass(va, path):
    rng = np.random.default_rng(43)
    n, dim, k = 4_099, 64, 5
    G = groups_per_pass() + 5
    assert G < (1 << 13)
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    tags = rng.integers(0, 1 << 13, n).astype(np.uint64) << np.uint64(51)              # 13 random bits, 51 .. 63
    rq = rng.standard_normal((G, dim)).astype(np.float32)
    v = (rng.permutation(1 << 13)[:G]).astype(np.uint64) << np.uint64(51)             # G distinct values: G distinct predicates
    preds = np.zeros((G, 3), np.uint64)
    preds[:, 1] = v                                                                    # all of the value's bits ...
    preds[::3, 0], preds[::3, 1] = v[::3], 0                                           # ... any of them for every third
    preds[::5, 2] = ~v[::5] & (np.uint64(3) << np.uint64(51))
    assert len(distinct_preds(preds)) == G and not (preds[:, 1] & preds[:, 2]).any()
    model = TagModelIndex(dim, "bf16", "cosine")
    model.add(raw)
    model.set_tags(0, tags)
    want = model.search_tagged(rq, k, preds)
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_tags(0, tags)
        ix.set_path(path)
        ids, sc = ix.search_tagged(rq, k, preds)
        st = ix.last_stats()
    print(path, st)
    assert_same(ids, sc, *want, f"{G} groups path{path}")
    if path == PATH_GATHER:
        assert st["path"] == PATH_GATHER and 1 <= st["scan_launches"] <= 2, st


# ---------------------------------------------------------------- launch count
def test_launch_count_does_not_grow_with_predicates(va):
    rng = np.random.default_rng(77)
    n, dim, k = 20_000, 64, 10
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    rq = rng.standard_normal((256, dim)).astype(np.float32)
    launches = {}
    for n_preds, qv in ((256, rng.permutation(256)), (4, rng.integers(0, 4, 256))):
        value = (rng.permutation(n) % n_preds).astype(np.uint64)                       # n_preds values in the low 8 bits
        tags = value | (rng.integers(0, 1 << 20, n).astype(np.uint64) << np.uint64(40))
        preds = np.zeros((256, 3), np.uint64)
        preds[:, 1] = qv.astype(np.uint64)                                             # the low 8 bits equal the value:
        preds[:, 2] = ~qv.astype(np.uint64) & np.uint64(0xFF)                          # all of its ones, none of its zeros
        model = TagModelIndex(dim, "bf16", "cosine")
        model.add(raw)
        model.set_tags(0, tags)
        with va.Index(dim, "bf16", "cosine") as ix:
            ix.add(raw)
            ix.set_tags(0, tags)
            ix.set_path(PATH_GATHER)
            ids, sc = ix.search_tagged(rq, k, preds)
            st = ix.last_stats()
        print(n_preds, st)
        assert_same(ids, sc, *model.search_tagged(rq, k, preds), f"{n_preds} predicates")
        assert st["path"] == PATH_GATHER
        launches[n_preds] = st["scan_launches"]
    assert launches[256] == launches[4] and 1 <= launches[256] <= 2, launches


# ---------------------------------------------------------------- ties by id
@pytest.mark.parametrize("path", [PATH_GATHER, PATH_AUTO, PATH_MFMA])
def test_ties_break_by_id_within_a_predicate(va, path):
    rng = np.random.default_rng(5)
    n, dim = 6_000, 64
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    tags = (np.uint64(1) << (np.arange(n) % 3 * 31 + 1).astype(np.uint64))            # bits 1, 32, 63 by r % 3
    same, other = [4000, 10, 997, 2500], [11, 2999]                                    # bit 32 rows (r % 3 == 1), bit 63 rows (r % 3 == 2)
    assert all(r % 3 == 1 for r in same) and all(r % 3 == 2 for r in other)
    v = rng.standard_normal(dim).astype(np.float32)
    raw[same + other] = v
    rq = np.stack([v, v, raw[7], v])
    preds = np.array([(B(32), 0, 0), (0, B(63), 0), (B(32), 0, 0), (B(32, 63), 0, B(1))], np.uint64)
    for dtype, metric in (("f32", "cosine"), ("bf16", "l2"), ("bf16", "ip")):
        model = TagModelIndex(dim, dtype, metric)
        model.add(raw)
        model.set_tags(0, tags)
        with va.Index(dim, dtype, metric) as ix:
            ix.add(raw)
            ix.set_tags(0, tags)
            ix.set_path(path)
            ids, sc = ix.search_tagged(rq, 6, preds)
        assert_same(ids, sc, *model.search_tagged(rq, 6, preds), f"{dtype}/{metric}")
        if metric != "ip":
            assert ids[0, :4].tolist() == sorted(same) and ids[1, :2].tolist() == sorted(other)
            assert ids[3, :6].tolist() == sorted(same + other)
        assert not set(ids[0].tolist()) & set(other) and not set(ids[1].tolist()) & set(same)


# ---------------------------------------------------------------- k beyond a group
@pytest.mark.parametrize("path", [PATH_GATHER, PATH_AUTO, PATH_STREAM])
def test_k_beyond_a_group(va, world, path):
    tags, corpora, queries, _ = world
    raw, rq = corpora[64], queries[64][:6]
    preds = np.array([P_ONE_ROW, (B(2), 0, 0), (B(4), 0, 0), P_ONE_ROW, P_NO_ROW, P_UNSAT], np.uint64)
    model = TagModelIndex(64, "bf16", "cosine")
    model.add(raw)
    model.set_tags(0, tags)
    with va.Index(64, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_tags(0, tags)
        ix.set_path(path)
        ids, sc = ix.search_tagged(rq, 100, preds)
        assert_same(ids, sc, *model.search_tagged(rq, 100, preds), "k=100")
        for q, rows in enumerate((1, 63, 65, 1, 0, 0)):
            assert (ids[q, :rows] != ID_NONE).all() and (ids[q, rows:] == ID_NONE).all() and np.isnan(sc[q, rows:]).all()
        p2 = np.array([(B(5), 0, 0), (B(3), 0, 0), (B(5), 0, 0)], np.uint64)
        ids, sc = ix.search_tagged(rq[:3], 3584, p2)
        assert_same(ids, sc, *model.search_tagged(rq[:3], 3584, p2), "k=3584")
        assert (ids[1, 64:] == ID_NONE).all() and (ids[0] != ID_NONE).all()


# ---------------------------------------------------------------- one long-lived handle against the model
@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "l2")])
def test_composition(va, world, dtype, metric):
    tags, corpora, queries, preds300 = world[0], world[1], world[2], world[3][300]
    n0, k, off = 30_001, 10, 1_000_000
    raw, rq = corpora[64][:n0], queries[64]
    rng = np.random.default_rng(9)
    model = TagModelIndex(64, dtype, metric)
    with va.Index(64, dtype, metric) as ix:
        def both(name, *args):
            getattr(model, name)(*args)
            return getattr(ix, name)(*args)

        def check(what, paths=(PATH_AUTO, PATH_GATHER)):
            assert ix.count == model.count
            assert np.array_equal(ix.get_tags(model.offset, model.count), model.tags), what
            want = model.search_tagged(rq, k, preds300)
            for path in paths:
                ix.set_path(path)
                ids, sc = ix.search_tagged(rq, k, preds300)
                assert_same(ids, sc, *want, f"{what} path{path}")
                check_stats(ix.last_stats(), path, dtype, 64, model, preds300, k, f"{what} path{path}")

        both("add", raw)
        ix.set_id_offset(off)
        model.offset = off
        both("set_tags", off + 5_000, tags[5_000:25_000])                             # a sub-range: the rest keeps 0
        check("sub-range", (PATH_AUTO,))
        both("set_tags", off, tags[:n0])
        one_row = model.matching(P_ONE_ROW)
        dead = np.unique(np.concatenate([rng.choice(n0, 2500, replace=False), model.matching((B(2), 0, 0))[:20], one_row,
                                         model.matching(p_pair(3))[:5]]))
        both("delete", dead.astype(np.uint64) + np.uint64(off))
        check("delete", (PATH_AUTO,))
        both("set_filter", rng.random(n0) < 0.7)
        check("filter + delete", (PATH_AUTO, PATH_GATHER, PATH_EXACT))
        live = np.flatnonzero(~model.deleted)
        upd = rng.choice(live, 500, replace=False)
        both("update", upd.astype(np.uint64) + np.uint64(off), rng.standard_normal((500, 64)).astype(np.float32))
        check("update keeps the tags", (PATH_AUTO,))
        both("add", rng.standard_normal((700, 64)).astype(np.float32))                 # tag 0, not allowed under the filter
        assert not ix.get_tags(off + n0, 700).any()
        check("add under a filter", (PATH_AUTO,))
        new_ids = ix.compact()
        assert np.array_equal(new_ids, model.compact())
        check("compact moves the tags")
        both("set_tags", off + 100, np.full(3_000, ALL_ONES, np.uint64))               # tags again, on the compacted rows
        both("set_filter", None)
        check("set_tags after compact")


# ---------------------------------------------------------------- defaults and errors
def test_defaults_and_errors(va, world):
    import torch
    tags, corpora, queries, _ = world
    n, k = 20_001, 10
    raw, rq = corpora[64][:n], queries[64][:40]
    model = TagModelIndex(64, "bf16", "cosine")
    model.add(raw)
    model.set_tags(0, tags[:n])
    with va.Index(64, "bf16", "cosine") as ix:
        ids, sc = ix.search_tagged(rq, k, np.zeros((40, 3), np.uint64))                 # an empty handle
        assert (ids == ID_NONE).all() and np.isnan(sc).all()
        ix.add(raw)
        ref = ix.search(rq, k)
        # tags never set: every row holds 0, so only predicates with any == all == 0 match
        never = np.array([(0, 0, 0), (0, 0, ALL_ONES), (0, 0, 1), (1, 0, 0), (0, 1 << 63, 0), (ALL_ONES, 0, 0), (0, 1, 2), (1, 0, 2)] * 5, np.uint64)
        ids, sc = ix.search_tagged(rq, k, never)
        sees = (never[:, 0] == 0) & (never[:, 1] == 0)
        assert_same(ids[sees], sc[sees], ref[0][sees], ref[1][sees], "unset tags, a predicate that asks for no bit")
        assert (ids[~sees] == ID_NONE).all() and np.isnan(sc[~sees]).all() and sees.sum() == 15
        assert not ix.get_tags(0, n).any()
        ix.set_tags(0, tags[:n])
        for first, m in ((n - 1, 2), (n + 1, 0), (n, 1), (1 << 40, 1)):               # not wholly within the rows: nothing changes
            with pytest.raises(va.VrodError) as e:
                ix.set_tags(first, np.full(m, 9, np.uint64))
            assert e.value.code == 1
            with pytest.raises(va.VrodError) as e:
                ix.get_tags(first, m)
            assert e.value.code == 1
        ix.set_tags(n, np.zeros(0, np.uint64))                                         # n == 0 does nothing
        assert np.array_equal(ix.get_tags(0, n), tags[:n])
        preds = np.array([P_HALF, P_TENTH, p_pair(7), P_EVERY] * 10, np.uint64)
        with pytest.raises(va.VrodError) as e:
            ix.search_tagged(rq, 3585, preds)                                          # k > VROD_MAX_K
        assert e.value.code == 1
        L, vp = ix._L, lambda a: a.ctypes.data
        oi, osc = np.zeros((40, k), np.uint64), np.zeros((40, k), np.float32)
        for args in ((None, vp(preds), vp(oi), vp(osc)), (vp(rq), None, vp(oi), vp(osc)), (vp(rq), vp(preds), None, vp(osc)),
                     (vp(rq), vp(preds), vp(oi), None)):
            assert L.vrod_search_tagged(ix._h, args[0], 40, k, args[1], args[2], args[3]) == 1
            assert L.vrod_search_tagged_device(ix._h, args[0], 40, k, args[1], args[2], args[3], None) == 1
        assert L.vrod_index_set_tags(ix._h, 0, None, 4) == 1 and L.vrod_index_get_tags(ix._h, 0, 4, None) == 1
        bad = rq.copy()
        bad[3, 5] = np.nan
        with pytest.raises(va.VrodError) as e:
            ix.search_tagged(bad, k, preds)
        assert e.value.code == 2
        want = model.search_tagged(rq, k, preds)
        assert_same(*ix.search_tagged(rq, k, preds), *want, "after the rejected calls")
        # a pending search blocks tags and tagged searches; after search_end both work
        dq = torch.from_numpy(rq).cuda()
        dp = torch.from_numpy(preds.view(np.int64)).cuda()
        doi = torch.empty((40, k), dtype=torch.int64, device="cuda")
        dsc = torch.empty((40, k), dtype=torch.float32, device="cuda")
        ix.search_begin_device(dq, k, doi, dsc)
        for call in (lambda: ix.search_tagged(rq, k, preds), lambda: ix.set_tags(0, tags[:10]), lambda: ix.search_tagged_device(dq, k, dp)):
            with pytest.raises(va.VrodError) as e:
                call()
            assert e.value.code == 1
        ix.search_end()
        assert_same(*ix.search_tagged(rq, k, preds), *want, "after search_end")
    with va.Index(64, "bf16", "cosine", devices=[0, 0]) as ix:
        ix.add(raw)
        with pytest.raises(va.VrodError) as e:
            ix.set_tags(0, tags[:n])
        assert e.value.code == 6
        oi, osc = np.full((40, k), 7, np.uint64), np.full((40, k), 7.0, np.float32)
        rc = ix._L.vrod_search_tagged(ix._h, rq.ctypes.data, 40, k, preds.ctypes.data, oi.ctypes.data, osc.ctypes.data)
        assert rc == 6 and (oi == 7).all() and (osc == 7.0).all()                      # outputs untouched
        assert not ix.get_tags(0, 100).any()


# ---------------------------------------------------------------- bystanders
def test_other_searches_ignore_tags(va, world):
    tags, corpora, queries, preds = world
    n, k = 20_001, 10
    raw, rq = corpora[100][:n], queries[100][:60]
    labels = (np.arange(n) % 7).astype(np.uint32)
    with va.Index(100, "f32", "l2") as ix:
        ix.add(raw)
        ix.set_labels(0, labels)

        def everything():
            out = [ix.search(rq, k), ix.search(rq[:3], k), ix.search_labeled(rq, k, np.arange(60) % 9), ix.search_grouped(rq[:20], 5)]
            out.append(ix.range_search(rq[:20], 150.0))
            out.append(ix.search_by_ids(np.arange(50, dtype=np.uint64) * 3, k))
            return out, ix.last_stats()
        before, st0 = everything()
        ix.set_tags(0, tags[:n])
        ix.search_tagged(rq, k, preds[300][:60])
        after, st1 = everything()
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        assert st0["scan_launches"] == st1["scan_launches"] and st0["path"] == st1["path"]
        assert np.array_equal(ix.get_labels(0, n), labels)


# ---------------------------------------------------------------- device form
def test_device_form_equals_host_form(va, world):
    import torch
    tags, corpora, queries, preds = world
    raw, rq, p, k = corpora[100], queries[100], preds[300], 10
    with va.Index(100, "bf16", "ip") as ix:
        ix.add(raw)
        ix.set_tags(0, tags)
        hi, hs = ix.search_tagged(rq, k, p)
        di, ds = ix.search_tagged_device(torch.from_numpy(rq).cuda(), k, torch.from_numpy(p.view(np.int64)).cuda())
        assert_same(di.cpu().numpy().view(np.uint64), ds.cpu().numpy(), hi, hs, "device form")
