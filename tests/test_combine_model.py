"""The model of vrod_search_combined (tests/combine_model.py) pinned on the CPU, so that the GPU tests which compare the
library with it can tell a reordered or a fused kernel from a correct one:

  - the vectorised combination equals a scalar loop over np.float32 values, bit for bit;
  - on the committed seed, permuting three terms changes the combined vector's bits (order is observable);
  - on the committed seed, an fp64 accumulate-then-round differs from it in at least one coordinate (fusing, or a wider
    accumulator, is observable);
  - the excluded set and the search over the remaining rows."""
import itertools

import numpy as np
import pytest

import combine_model as M
from support import DT, ID_NONE, O, bits, prep_of  # noqa: F401

SEED = 20240611   # both premises below hold on it; if an edit breaks one, pick another here


def small(O, dtype, metric, n=40, dim=5, seed=SEED):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    return rng, raw, O.prepare(raw, DT[dtype], prep_of(metric), threads=1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
def test_vectorised_combination_equals_the_scalar_loop(O, dtype, metric):
    rng, raw, pc = small(O, dtype, metric)
    for case in range(20):
        nt = int(rng.integers(0, 6))
        terms = rng.integers(0, raw.shape[0], nt)
        weights = rng.uniform(-1, 1, nt).astype(np.float32)
        vector = rng.standard_normal(5).astype(np.float32) if case % 2 or nt == 0 else None
        vw = None if case % 4 < 2 else float(rng.uniform(-2, 2))
        a = M.combine(O, pc, dtype, metric, vector, vw, terms, weights)
        b = M.combine_scalar(O, pc, dtype, metric, vector, vw, terms, weights)
        assert a.dtype == np.float32 and np.array_equal(bits(a), bits(b)), case


def test_combination_starts_from_plus_zero_and_keeps_the_order():
    pc = np.array([[-0.0, 1.0], [0.0, 1e-8]], np.float32)
    # +0 + fl(1 * -0) = +0: a single term of weight 1 whose coordinate is -0 gives +0, not the stored bits
    assert bits(M.combine(None, pc, "f32", "l2", None, None, [0], [1.0])).tolist() == [0, bits(np.float32(1.0))]
    # (1 + 1e-8) - 1 = 0 but (1 - 1) + 1e-8 = 1e-8
    a = M.combine(None, np.array([[1.0], [1e-8], [1.0]], np.float32), "f32", "l2", None, None, [0, 1, 2], [1, 1, -1])
    b = M.combine(None, np.array([[1.0], [1e-8], [1.0]], np.float32), "f32", "l2", None, None, [0, 2, 1], [1, -1, 1])
    assert a[0] == 0 and b[0] == np.float32(1e-8)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_order_and_fusing_are_observable_on_the_committed_seed(O, dtype):
    """The two premises of the GPU tests: at the shapes they use (d = 72, three terms with weights in [-1, 1]) a permutation
    of the terms, and an fp64 accumulate-then-round, each change at least one bit of the combined vector."""
    rng = np.random.default_rng(SEED)
    raw = rng.standard_normal((64, 72)).astype(np.float32)
    pc = O.prepare(raw, DT[dtype], prep_of("cosine"), threads=1)
    terms = [3, 17, 41]
    weights = rng.uniform(-1, 1, 3).astype(np.float32)
    base = M.combine(O, pc, dtype, "cosine", None, None, terms, weights)
    changed = 0
    for perm in itertools.permutations(range(3)):
        if perm == (0, 1, 2):
            continue
        p = M.combine(O, pc, dtype, "cosine", None, None, [terms[i] for i in perm], [weights[i] for i in perm])
        changed += not np.array_equal(bits(p), bits(base))
        assert np.allclose(p, base, rtol=0, atol=1e-6)
    assert changed >= 3, "permuting the terms must change the combined vector's bits"
    wide = M.combine_fp64(O, pc, dtype, "cosine", None, None, terms, weights)
    assert (bits(wide) != bits(base)).sum() >= 1, "an fp64 accumulate-then-round must differ in at least one coordinate"
    assert np.allclose(wide, base, rtol=0, atol=1e-6)


def test_excluded_set_and_search(O):
    rng, raw, pc = small(O, "f32", "l2", n=30)
    elig = np.setdiff1d(np.arange(30), [4, 9])
    queries = [
        {"terms": [1, 2], "weights": [1.0, -0.5]},
        {"terms": [3], "weights": [1.0], "exclude": [3, 3, 4, 1000, int(ID_NONE), 7]},
        {"vector": raw[5] * 2, "vw": 0.5, "terms": [], "weights": []},
    ]
    off = 100
    for Q in queries:
        Q["exclude"] = [x + off if x < 30 else x for x in Q.get("exclude", ())]
    assert M.excluded_ids(queries[0], True, off) == [101, 102] and M.excluded_ids(queries[0], False, off) == []
    ids, sc = M.search(O, raw, pc, "f32", "l2", queries, 28, elig, exclude_terms=True, id_offset=off)
    assert ids.shape == (3, 28)
    filled = (ids != ID_NONE).sum(axis=1).tolist()
    assert filled == [26, 26, 28]                       # 28 eligible rows minus {1, 2}, minus {3, 7} (4 is not eligible anyway)
    assert not np.isin(ids[0], [101, 102]).any() and not np.isin(ids[1], [103, 107]).any()
    assert not np.isin(ids, [104, 109]).any()
    # the survivors are the unexcluded ranking with the excluded ids struck out
    full, _ = M.search(O, raw, pc, "f32", "l2", [{"terms": [3], "weights": [1.0]}], 28, elig, id_offset=off)
    want = [i for i in full[0].tolist() if i not in (103, 107)]
    assert ids[1, :26].tolist() == want[:26]
    # l2, one term of weight 1: the query is the stored row, so without the flag the row itself comes first at distance +0
    assert full[0, 0] == 103
    # flat(): the C arguments
    vec, vw, tl, tid, tw, xl, xid = M.flat(queries[:2])
    assert vec is None and vw is None and tl.tolist() == [0, 2, 3] and tid.tolist() == [1, 2, 3] and xl.tolist() == [0, 0, 6]
    assert xid.dtype == np.uint64 and xid[-2] == ID_NONE
