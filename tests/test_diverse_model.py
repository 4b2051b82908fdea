"""Properties of the diversified search's model (tests/diverse_model.py) -- no GPU, no library: what the GPU tests compare
against must itself be MMR.

  - lambda = 1 is the plain search: the first k of the pool, in order, bit for bit;
  - pool == k returns a permutation of the plain top k (there is nothing else to pick from), starting with its best row;
  - on 20 tight clusters of 10 near-copies, a query at one cluster's centre gets its plain top 10 from that one cluster
    (the premise) and strictly more clusters under k = 10, pool = 100, lambda = 0.5 -- for every metric and storage type;
  - the greedy rules on hand-made inputs: ties by position, NaN last, -0.0 == +0.0, pen's NaN rule.
"""
import numpy as np
import pytest

import diverse_model as DM
from support import ID_NONE, bits

D = 24


def gaussian_index(dtype, metric, n=400, seed=5):
    rng = np.random.default_rng(seed)
    ix = DM.DiverseModel(D, dtype, metric)
    ix.add(rng.standard_normal((n, D)).astype(np.float32))
    return ix, rng.standard_normal((6, D)).astype(np.float32)


@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lambda_one_is_the_plain_search(dtype, metric):
    ix, rq = gaussian_index(dtype, metric)
    ids, sc, mmr = ix.search_diverse(rq, 12, 50, 1.0)
    oi, osc = ix.search(rq, 12)
    assert np.array_equal(ids, oi) and np.array_equal(bits(sc), bits(osc))
    assert np.array_equal(mmr, sc)                 # fl(1 * r - 0 * pen) = r on finite scores (as values: -0 may turn +0)


@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.5])
def test_pool_equal_k_is_a_permutation_of_the_top_k(metric, lam):
    ix, rq = gaussian_index("f32", metric)
    k = 15
    ids, sc, _ = ix.search_diverse(rq, k, k, lam)
    oi, osc = ix.search(rq, k)
    assert np.array_equal(ids[:, 0], oi[:, 0])     # step 0 takes position 0
    for q in range(rq.shape[0]):
        o = np.argsort(ids[q], kind="stable")
        p = np.argsort(oi[q], kind="stable")
        assert np.array_equal(ids[q][o], oi[q][p]) and np.array_equal(bits(sc[q][o]), bits(osc[q][p]))
    assert not np.array_equal(ids, oi)             # ... and lambda < 1 does reorder some of them


@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_near_duplicate_clusters_are_spread(dtype, metric):
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((20, D)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows = (np.repeat(centres, 10, axis=0) + 0.01 * rng.standard_normal((200, D))).astype(np.float32)
    cluster = np.repeat(np.arange(20), 10)
    ix = DM.DiverseModel(D, dtype, metric)
    ix.add(rows)
    rq = centres[7:8]
    plain, _ = ix.search(rq, 10)
    assert set(cluster[plain[0].astype(np.int64)]) == {7}, "premise: the plain top 10 sits in the query's cluster"
    ids, _, _ = ix.search_diverse(rq, 10, 100, 0.5)
    assert (ids != ID_NONE).all() and np.unique(ids).size == 10
    assert len(set(cluster[ids[0].astype(np.int64)])) > 1
    assert ids[0, 0] == plain[0, 0]


def test_unfilled_slots_and_short_pools():
    ix = DM.DiverseModel(D, "f32", "cosine", id_offset=1000)
    rng = np.random.default_rng(2)
    rq = rng.standard_normal((2, D)).astype(np.float32)
    ids, sc, mmr = ix.search_diverse(rq, 5, 8, 0.5)          # an empty handle
    assert (ids == ID_NONE).all() and np.isnan(sc).all() and np.isnan(mmr).all()
    ix.add(rng.standard_normal((3, D)).astype(np.float32))
    ids, sc, mmr = ix.search_diverse(rq, 5, 8, 0.5)
    assert (ids[:, :3] >= 1000).all() and (ids[:, 3:] == ID_NONE).all()
    assert not np.isnan(sc[:, :3]).any() and np.isnan(sc[:, 3:]).all() and np.isnan(mmr[:, 3:]).all()
    for q in range(2):
        assert sorted(ids[q, :3]) == [1000, 1001, 1002]


def test_greedy_rules_on_hand_made_inputs():
    f = np.float32
    nan = f(np.nan)
    # every r and g equal: v ties at every step and the position decides
    r = np.full(5, 0.5, f)
    G = np.full((5, 5), 0.25, f)
    pos, v = DM.greedy(r, G, 5, 0.5, False)
    assert pos.tolist() == [0, 1, 2, 3, 4]
    assert v.tolist() == [0.25] + [f(f(0.5) * f(0.5)) - f(f(0.5) * f(0.25))] * 4
    # higher is better: position 2 is a copy of 0 (g = 1), position 1 is unrelated (g = 0)
    r = np.array([0.9, 0.5, 0.9], f)
    G = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]], f)
    assert DM.greedy(r, G, 3, 0.5, False)[0].tolist() == [0, 1, 2]
    assert DM.greedy(r, G, 3, 1.0, False)[0].tolist() == [0, 2, 1]
    # lower is better (l2): position 1 is at distance 0 from 0, position 2 is far from it
    r = np.array([1.0, 1.0, 2.0], f)
    G = np.array([[0, 0, 9], [0, 0, 9], [9, 9, 0]], f)
    assert DM.greedy(r, G, 3, 0.5, True)[0].tolist() == [0, 2, 1]
    # a NaN v loses to any number; an all-NaN step goes to the smallest position
    r = np.array([1.0, nan, 0.1, nan], f)
    G = np.zeros((4, 4), f)
    pos, v = DM.greedy(r, G, 4, 0.5, False)
    assert pos.tolist() == [0, 2, 1, 3] and np.isnan(v[2:]).all()
    # a NaN g loses to any number: pen of position 1 is g(1, 2) = 0.5 although g(1, 0) is NaN; pen stays NaN (and v NaN)
    # only while every g is NaN
    r = np.array([1.0, 0.8, 0.9], f)
    G = np.array([[1, nan, 0.1], [nan, 1, 0.5], [0.1, 0.5, 1]], f)
    pos, v = DM.greedy(r, G, 3, 0.5, False)
    assert pos.tolist() == [0, 2, 1]
    assert v[2] == f(f(0.5) * f(0.8)) - f(f(0.5) * f(0.5))
    # -0.0 == +0.0: lambda = 0 and r = -0, +0 give v = (-0) - (+0) = -0 and (+0) - (+0) = +0 -- a tie, position 1 first
    r = np.array([1.0, -0.0, 0.0], f)
    G = np.zeros((3, 3), f)
    pos, v = DM.greedy(r, G, 2, 0.0, False)
    assert pos.tolist() == [0, 1] and np.signbit(v[1])
    assert DM.greedy(r, G, 2, 0.0, True)[0].tolist() == [0, 1]


def test_check_args_mirror():
    assert DM.check_args(0, 5, 0.5) == 1 and DM.check_args(6, 5, 0.5) == 2 and DM.check_args(5, 1025, 0.5) == 3
    assert DM.check_args(5, 5, -0.1) == 4 and DM.check_args(5, 5, 1.1) == 4 and DM.check_args(5, 5, float("nan")) == 4
    assert DM.check_args(5, 5, 0.0) == 0 and DM.check_args(1024, 1024, 1.0) == 0
