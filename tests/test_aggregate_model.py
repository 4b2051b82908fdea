"""aggregate_model.AggregateModelIndex against a row-by-row Python loop over Python ints: the three key rules, the five
aggregates with the sum reduced mod 2^64 by hand, and the two orders.  No device and no library."""
import numpy as np
import pytest

from aggregate_model import AGG_GROUP_DTYPE, BY_LABEL, BY_TAG, BY_VALUE, ERR_CAPACITY, MAX_AGG_GROUPS, ORDER_COUNT, AggregateModelIndex, by_count, fold
from index_model import ERR_INVALID_ARG, ModelError
from rowpred_model import ALLOWED, MATCH_ALL
from where_model import I64_MAX, I64_MIN

DIM = 4
U64 = (1 << 64) - 1


def signed(x):
    x &= U64
    return x - (1 << 64) if x >> 63 else x


def loop(m, pred, by, width, flags):
    """The literal definition, one row at a time -> ({key: [count, min, max, sum, first_id]}, rows)."""
    groups, rows = {}, 0
    for r in m.matching(pred, flags & ALLOWED).tolist():
        rows += 1
        v, t, rid = int(m.values[r]), int(m.tags[r]), r + m.offset
        if by == BY_LABEL:
            keys = [int(m.labels[r])]
        elif by == BY_VALUE:
            keys = [v // width]                                                  # Python's // floors
        else:
            keys = [b for b in range(64) if (t >> b) & 1]
        for k in keys:
            g = groups.setdefault(k, [0, I64_MAX, I64_MIN, 0, U64])
            g[0] += 1
            g[1], g[2] = min(g[1], v), max(g[2], v)
            g[3] = signed(g[3] + v)                                              # wraps mod 2^64
            g[4] = min(g[4], rid)
    return groups, rows


def expect(groups, flags):
    items = sorted(groups.items(), key=(lambda kv: (-kv[1][0], kv[0])) if flags & ORDER_COUNT else (lambda kv: kv[0]))
    return [(k, *g) for k, g in items]


def handle(n, off=0, seed=0):
    rng = np.random.default_rng(seed)
    m = AggregateModelIndex(DIM, "f32", "l2", id_offset=off)
    m.add(rng.standard_normal((n, DIM)).astype(np.float32))
    return m, rng


def check(m, pred, by, width, flags=0):
    got, n_groups, n_rows = m.aggregate_where(pred, by, width, None, flags)
    want, rows = loop(m, pred, by, width, flags)
    assert got.dtype == AGG_GROUP_DTYPE and got.tolist() == expect(want, flags)
    assert n_groups == len(want) and n_rows == rows
    for limit in (0, 1, n_groups, n_groups + 3):
        cut, g2, r2 = m.aggregate_where(pred, by, width, limit, flags)
        assert cut.tolist() == got[:limit].tolist() and (g2, r2) == (n_groups, n_rows)
    return got


def test_floor_division_on_negative_values():
    m, rng = handle(400, off=50)
    vals = rng.integers(-100, 100, 400)
    vals[:8] = [-1, 0, 1, -10, -11, 9, 10, -9]
    m.set_values(50, vals)
    got = check(m, MATCH_ALL, BY_VALUE, 10)
    assert -1 in got["key"] and got["key"].min() == -10                          # -1 // 10 == -1, not 0
    for width in (1, 2, 86400, I64_MAX):
        check(m, MATCH_ALL, BY_VALUE, width)
        check(m, MATCH_ALL, BY_VALUE, width, ORDER_COUNT)


def test_the_extremes_and_sums_that_wrap():
    m, _ = handle(64)
    vals = np.array([I64_MIN, -1, 0, I64_MAX] * 16, np.int64)
    vals[4:8] = [I64_MAX, I64_MAX, I64_MIN, I64_MIN]
    m.set_values(0, vals)
    m.set_labels(0, np.arange(64, dtype=np.uint32) % 3)
    got = check(m, MATCH_ALL, BY_VALUE, 1)
    assert got["key"].tolist() == [I64_MIN, -1, 0, I64_MAX]                      # every int64 is a key under width 1
    assert got["sum_value"][3] == signed(I64_MAX * int(got["count"][3]))         # 17 * INT64_MAX wrapped
    got = check(m, MATCH_ALL, BY_VALUE, I64_MAX)
    assert got["key"].tolist() == [-2, -1, 0, 1]                                 # INT64_MIN // INT64_MAX == -2
    check(m, MATCH_ALL, BY_VALUE, 2)
    check(m, MATCH_ALL, BY_VALUE, 86400)
    by_label = check(m, MATCH_ALL, BY_LABEL, None)
    assert sum(int(x) for x in by_label["count"]) == 64 and (by_label["min_value"] == I64_MIN).all() and (by_label["max_value"] == I64_MAX).all()


def test_tags_zero_one_bit_and_all_ones():
    m, rng = handle(200, off=7)
    tags = np.zeros(200, np.uint64)
    tags[::4] = np.uint64(1) << rng.integers(0, 64, 50).astype(np.uint64)
    tags[1::4] = np.uint64(U64)
    tags[2::4] = rng.integers(0, 1 << 63, 50).astype(np.uint64) | np.uint64(1 << 63)
    m.set_tags(7, tags)
    m.set_values(7, rng.integers(I64_MIN, I64_MAX, 200, endpoint=True))
    for flags in (0, ORDER_COUNT):
        got = check(m, MATCH_ALL, BY_TAG, None, flags)
        assert got.size == 64
        assert sum(int(x) for x in got["count"]) == sum(bin(int(t)).count("1") for t in tags)
    _, _, rows = m.aggregate_where(MATCH_ALL, BY_TAG)
    assert rows == 200                                                           # the rows without tags are considered, in no group
    m.set_tags(7, np.zeros(200, np.uint64))
    got, groups, rows = m.aggregate_where(MATCH_ALL, BY_TAG)
    assert (got.size, groups, rows) == (0, 0, 200)


def test_count_ties_under_order_count():
    m, _ = handle(12)
    m.set_labels(0, np.array([5, 5, 9, 9, 1, 1, 7, 3, 3, 3, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32))
    got = check(m, MATCH_ALL, BY_LABEL, None, ORDER_COUNT)
    assert got["key"].tolist() == [3, 1, 5, 9, 0xFFFFFFFF, 7]                    # 3 rows; four ties at 2 by key; 1 row
    assert check(m, MATCH_ALL, BY_LABEL, None)["key"].tolist() == [1, 3, 5, 7, 9, 0xFFFFFFFF]
    g = np.zeros(3, AGG_GROUP_DTYPE)
    g["key"], g["count"] = [-5, 2, -7], [1, (1 << 64) - 1, 1]
    assert by_count(g)["key"].tolist() == [2, -7, -5]                            # counts are unsigned, keys signed


def test_scope_predicate_and_offset():
    m, rng = handle(300, off=1000, seed=3)
    m.set_values(1000, rng.integers(-50, 50, 300))
    m.set_tags(1000, rng.integers(0, 16, 300).astype(np.uint64))
    m.set_labels(1000, rng.integers(0, 5, 300).astype(np.uint32))
    m.set_filter(rng.random(300) < 0.7)
    m.delete(np.arange(1000, 1300, 9, dtype=np.uint64))
    for pred in (MATCH_ALL, (3, 0, 8, -20, 30, 0, 0), (0, 0, 0, I64_MIN, I64_MAX, 2, 1), (0, 1, 1, I64_MIN, I64_MAX, 0, 0)):
        for flags in (0, ALLOWED, ORDER_COUNT, ALLOWED | ORDER_COUNT):
            for by, width in ((BY_LABEL, None), (BY_VALUE, 7), (BY_TAG, None)):
                got = check(m, pred, by, width, flags)
                assert got.size == 0 or got["first_id"].min() >= 1000
    assert m.aggregate_where((0, 0, 0, I64_MIN, I64_MAX, 2, 1), BY_LABEL)[0]["key"].tolist() == [2]


def test_refusals_and_the_cap():
    m, _ = handle(5)
    for args in ((MATCH_ALL, BY_LABEL, None, None, 2), (MATCH_ALL, BY_LABEL, None, None, 8), (MATCH_ALL, 3, None), (MATCH_ALL, BY_VALUE, 0),
                 (MATCH_ALL, BY_VALUE, -1), (MATCH_ALL, BY_VALUE, None), ((0, 0, 0, 0, 0, 0, 2), BY_LABEL)):
        with pytest.raises(ModelError) as e:
            m.aggregate_where(*args)
        assert e.value.code == ERR_INVALID_ARG
    keys = np.arange(MAX_AGG_GROUPS + 1, dtype=np.int64)
    assert fold(keys[:-1], keys[:-1], keys[:-1].astype(np.uint64)).size == MAX_AGG_GROUPS
    big = AggregateModelIndex(DIM, "f32", "l2")
    big.add(np.zeros((MAX_AGG_GROUPS + 1, DIM), np.float32))
    big.set_labels(0, keys.astype(np.uint32))
    with pytest.raises(ModelError) as e:
        big.aggregate_where(MATCH_ALL, BY_LABEL)
    assert e.value.code == ERR_CAPACITY
