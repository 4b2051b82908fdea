"""CPU tests of tests/centroid_model.py, the restatement of vrod_index_centroids_where that the GPU tests compare with:
the properties the definition promises, checked on the model itself with Python ints and fp64."""
from fractions import Fraction

import numpy as np
import pytest

import centroid_model as CM
from aggregate_model import BY_LABEL, BY_VALUE
from rowpred_model import ALLOWED, MATCH_ALL

F32_MAX = np.float32(3.4028234663852886e38)


def ulp32(v):
    """The spacing of float32 at |v| (an array): the distance to the next float32 above |v|."""
    a = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)).astype(np.float64) - a.astype(np.float64))


def below_pow2(E):
    """The largest fp32 below 2^E."""
    return np.nextafter(np.float32(np.ldexp(1.0, E)), np.float32(0))


def test_row_bits_steps_between_4095_and_4096():
    assert [CM.row_bits(n) for n in (0, 1, 2, 3, 4, 4095, 4096, 4097, (1 << 32) - 1, 1 << 32)] == [0, 1, 2, 2, 3, 12, 13, 13, 32, 33]
    for n in (1, 5, 4095, 4096, 10_000_000):
        R = CM.row_bits(n)
        assert n < (1 << R) and (R == 0 or n >= (1 << (R - 1)))
    assert CM.scale(4095, 1) == 49 and CM.scale(4096, 1) == 48


def test_exponent_bounds_every_element():
    for m, E in ((0, -125), (1, -125), (0x007FFFFF, -125), (0x00800000, -125), (0x00FFFFFF, -125), (0x01000000, -124), (0x3F800000, 1),
                 (0x3FFFFFFF, 1), (0x40000000, 2), (0x7F7FFFFF, 128)):
        assert CM.exponent(m) == E
        x = np.array([m], np.uint32).view(np.float32)[0]
        assert float(x) < 2.0 ** E and (m < 0x01000000 or float(x) >= 2.0 ** (E - 1))


def test_permuting_a_groups_rows_changes_no_bit():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((700, 9)) * np.exp(rng.uniform(-30, 30, (700, 9)))).astype(np.float32)
    keys = rng.integers(-3, 4, 700).astype(np.int64)
    for cosine, sums in ((False, False), (False, True)):
        k0, c0, v0 = CM.centroids(x, keys, 700, cosine, sums)
        for seed in range(5):
            p = np.random.default_rng(seed).permutation(700)
            k1, c1, v1 = CM.centroids(x[p], keys[p], 700, cosine, sums)
            assert np.array_equal(k0, k1) and np.array_equal(c0, c1) and v0.tobytes() == v1.tobytes()


@pytest.mark.parametrize("E", [-125, 0, 1, 128])
@pytest.mark.parametrize("R", [1, 5, 12])
def test_no_wrap_at_the_edge(R, E):
    """2^R - 1 rows in one group, every element the largest fp32 below 2^E: |S| < 2^62 in Python ints, and the int64 sum
    of the model is that number."""
    n = (1 << R) - 1
    big = below_pow2(E)
    assert CM.row_bits(n) == R and CM.exponent(int(CM.abs_bits(big))) == E
    s = CM.scale(n, E)
    for sign in (1, -1):
        x = np.full((n, 2), sign * big, np.float32)
        q = CM.quantise(x, s)
        assert all(abs(int(v)) <= 1 << (62 - R) for v in q.reshape(-1))
        S = sum(int(v) for v in q[:, 0])
        assert abs(S) < 1 << 62
        _, counts, sums = CM.centroids(x, np.zeros(n, np.int64), n, False, True)
        assert counts.tolist() == [n] and sums[0, 0] == np.float32(np.float64(S) * 2.0 ** -s)
        assert int(np.add.reduce(q[:, 0])) == S                                  # the int64 reduction did not wrap
        _, _, means = CM.centroids(x, np.zeros(n, np.int64), n, False, False)
        assert means[0, 0] == sign * big                                         # the mean of equal rows is the row


def test_quantise_rounds_ties_to_even_and_is_exact_above_the_quantum():
    # with s = 0 the quantum is 1: halves go to the even neighbour, whatever the sign
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, 0.50000006, 3.0, -0.0, 0.0], np.float32)
    assert CM.quantise(x, 0).tolist() == [0, 2, 2, 0, -2, -2, 0, 1, 3, 0, 0]
    rng = np.random.default_rng(2)
    x = rng.standard_normal(1000).astype(np.float32)
    for s in (3, 30, 49):                                                        # |x| < 2^3 here, well inside int64
        q = CM.quantise(x, s)
        for v, k in zip(x[:200], q[:200]):
            num, den = float(v).as_integer_ratio()                               # x * 2^s as an exact rational
            err = Fraction(num << s, den) - int(k)
            assert abs(err) <= Fraction(1, 2) and (abs(err) < Fraction(1, 2) or int(k) % 2 == 0)
        assert s < 30 or all(Fraction(float(v)) * (1 << s) == int(k) for v, k in zip(x[:200], q[:200]) if abs(v) >= 2.0 ** -6)   # 24 bits fit


def test_against_an_fp64_mean():
    """|out - mean64| <= 2^-s + ulp32(mean64): half a quantum per element, which the mean keeps, plus the two roundings."""
    rng = np.random.default_rng(3)
    n = 3000
    for scale_up, cosine in ((1.0, True), (1.0, False), (1e30, False), (1e-30, False)):
        x = (rng.standard_normal((n, 16)) * scale_up).astype(np.float32)
        if cosine:
            x /= np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True).astype(np.float32) * np.float32(1.0001)
        keys = rng.integers(0, 11, n).astype(np.int64)
        uniq, counts, means = CM.centroids(x, keys, n, cosine, False)
        _, _, sums = CM.centroids(x, keys, n, cosine, True)
        E = 1 if cosine else CM.exponent(int(CM.abs_bits(x).max()))
        quantum = 2.0 ** -CM.scale(n, E)
        for g, k in enumerate(uniq):
            mean64 = x[keys == k].astype(np.float64).mean(axis=0)
            sum64 = x[keys == k].astype(np.float64).sum(axis=0)
            assert (np.abs(means[g].astype(np.float64) - mean64) <= quantum + ulp32(mean64)).all()
            assert (np.abs(sums[g].astype(np.float64) - sum64) <= float(counts[g]) * quantum + ulp32(sum64) + 1e-9 * np.abs(sum64)).all()


def test_a_row_and_its_negation_sum_to_plus_zero():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((40, 7)) * np.exp(rng.uniform(-80, 80, (40, 7)))).astype(np.float32)
    x[3] = -0.0
    both = np.concatenate([x, -x])
    for sums in (False, True):
        _, counts, v = CM.centroids(both, np.zeros(80, np.int64), 80, False, sums)
        assert counts.tolist() == [80] and (v.view(np.uint32) == 0).all()        # +0.0, never -0.0
    _, _, v = CM.centroids(np.full((3, 2), -0.0, np.float32), np.zeros(3, np.int64), 3, False, False)
    assert (v.view(np.uint32) == 0).all()


def test_non_finite_rows_are_refused_only_when_considered():
    x = np.ones((4, 3), np.float32)
    x[2, 1] = np.inf
    with pytest.raises(CM.ModelError) as e:
        CM.centroids(x, np.zeros(4, np.int64), 4, False, False)
    assert e.value.code == CM.ERR_INVALID_ARG
    keep = np.array([0, 1, 3])
    assert CM.centroids(x[keep], np.zeros(3, np.int64), 4, False, False)[2].tolist() == [[1.0, 1.0, 1.0]]


def test_the_model_index_groups_as_aggregate_where_does():
    rng = np.random.default_rng(5)
    n, dim, off = 500, 6, 1000
    m = CM.CentroidModelIndex(dim, "f32", "l2", id_offset=off)
    m.add(rng.standard_normal((n, dim)).astype(np.float32))
    labels = rng.integers(0, 9, n).astype(np.uint32)
    values = rng.integers(-50, 50, n).astype(np.int64)
    m.set_labels(off, labels)
    m.set_values(off, values)
    m.set_filter(rng.random(n) < 0.7)
    m.delete(np.arange(off, off + n, 7, dtype=np.uint64))
    for by, width in ((BY_LABEL, None), (BY_VALUE, 7)):
        for flags in (0, ALLOWED, CM.CENTROID_SUM, ALLOWED | CM.CENTROID_SUM):
            groups, vectors, n_rows = m.centroids_where(MATCH_ALL, by, width, None, flags)
            agg, n_groups, agg_rows = m.aggregate_where(MATCH_ALL, by, width, None, flags & ALLOWED)
            assert n_rows == agg_rows and groups.size == n_groups and vectors.shape == (n_groups, dim)
            assert all(np.array_equal(groups[f], agg[f]) for f in ("key", "count", "first_id"))
            assert groups["first_id"].min() >= off + 1                           # row 0 is deleted; ids carry the offset
            rows = m.matching(MATCH_ALL, flags & ALLOWED)
            key = labels[rows].astype(np.int64) if by == BY_LABEL else values[rows] // 7
            g = 2
            want = m.prepared()[rows][key == groups["key"][g]].astype(np.float64)
            want = want.sum(axis=0) if flags & CM.CENTROID_SUM else want.mean(axis=0)
            assert np.allclose(vectors[g], want, rtol=1e-6, atol=1e-6)
    with pytest.raises(CM.ModelError) as e:
        m.centroids_where(MATCH_ALL, BY_LABEL, None, 3, 0)
    assert e.value.code == CM.ERR_CAPACITY
    for bad in (dict(by=2), dict(by=BY_VALUE, width=0), dict(by=BY_LABEL, flags=2), dict(by=BY_LABEL, flags=4), dict(by=BY_LABEL, capacity=0),
                dict(by=BY_LABEL, capacity=CM.MAX_CENTROID_GROUPS + 1)):
        with pytest.raises(CM.ModelError) as e:
            m.centroids_where(MATCH_ALL, **bad)
        assert e.value.code == CM.ERR_INVALID_ARG
    assert m.centroids_where((0, 1, 1, 0, 0, 0, 0), BY_LABEL)[0].size == 0       # unsatisfiable: no groups
