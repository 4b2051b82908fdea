"""order_model.OrderModelIndex against a literal Python sorted() over (value, id) tuples, on small random handles: both
directions, cursors of every kind (none, a row's own, inside a tie class, a deleted row's, below the offset, beyond the
count, UINT64_MAX, before the first and past the last row), limit 0, and the scope flags."""
import numpy as np
import pytest

from index_model import ModelError
from order_model import DESC, MAX_ORDERED, OrderModelIndex
from rowpred_model import ALLOWED, MATCH_ALL
from where_model import I64_MAX, I64_MIN

U64_MAX = (1 << 64) - 1
VALUES = [I64_MIN, I64_MIN + 1, -1, 0, 1, 2, I64_MAX - 1, I64_MAX]


def handle(seed, n=90, off=0):
    rng = np.random.default_rng(seed)
    m = OrderModelIndex(4, "f32", "l2", id_offset=off)
    m.add(rng.standard_normal((n, 4)).astype(np.float32))
    m.set_values(off, np.array(VALUES, np.int64)[rng.integers(0, len(VALUES), n)])
    m.set_tags(off, rng.integers(0, 4, n).astype(np.uint64))
    m.set_labels(off, rng.integers(0, 3, n).astype(np.uint32))
    m.set_filter(rng.random(n) < 0.7)
    m.delete(rng.choice(n, 12, replace=False).astype(np.uint64) + np.uint64(off))
    return m


def literal(m, pred, limit, desc, after, flags):
    """The contract of include/vrod.h spelled out row by row."""
    out = []
    for r in range(m.count):
        if m.deleted[r] or (flags & ALLOWED and m.allow is not None and not m.allow[r]):
            continue
        t, v, l = int(m.tags[r]), int(m.values[r]), int(m.labels[r])
        a, b, c, lo, hi, label, has = (int(x) for x in pred)
        if not ((a == 0 or t & a) and t & b == b and t & c == 0 and lo <= v <= hi and (not has or l == label)):
            continue
        i = r + m.offset
        if after is not None:
            cv, cid = after
            if not ((v < cv if desc else v > cv) or (v == cv and i > cid)):
                continue
        out.append((v, i))
    out = sorted(out, key=lambda e: (-e[0], e[1]) if desc else e)
    return [e[1] for e in out[:limit]], [e[0] for e in out[:limit]], len(out)


PREDS = [MATCH_ALL, (1, 0, 0, I64_MIN, I64_MAX, 0, 0), (0, 0, 2, -1, I64_MAX, 1, 1), (0, 0, 0, I64_MIN, 0, 0, 0), (0, 1, 1, I64_MIN, I64_MAX, 0, 0),
         (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 3, 1000, 0, 0)]


@pytest.mark.parametrize("seed,off", [(1, 0), (2, 1000)])
def test_the_model_is_the_literal_contract(seed, off):
    m = handle(seed, off=off)
    dead = int(np.flatnonzero(m.deleted)[0]) + off
    live = int(np.flatnonzero(~m.deleted)[5])
    cursors = [None, (int(m.values[live]), live + off), (0, off + 40), (1, dead), (int(m.values[dead - off]), dead), (0, 0), (-1, off + m.count),
               (2, off + m.count + 7), (0, U64_MAX), (I64_MIN, 0), (I64_MAX, 0), (I64_MIN, U64_MAX), (I64_MAX, U64_MAX), (I64_MAX - 1, 3)]
    seen = 0
    for pred in PREDS:
        for flags in (0, ALLOWED):
            for desc in (False, True):
                for after in cursors:
                    for limit in (0, 1, 7, 90, 200):
                        ids, vals, total = m.select_ordered(pred, limit, desc, after, flags)
                        assert ids.dtype == np.uint64 and vals.dtype == np.int64
                        assert (ids.tolist(), vals.tolist(), total) == literal(m, pred, limit, desc, after, flags), (pred, flags, desc, after, limit)
                        seen += total > 0
                        assert m.select_ordered(pred, limit, False, after, flags | (DESC if desc else 0))[0].tolist() == ids.tolist()
    assert seen > 500


def test_pages_concatenate_to_the_listing():
    m = handle(3, n=120)
    for desc in (False, True):
        whole = m.select_ordered(MATCH_ALL, 200, desc)
        pages = list(m.scroll(MATCH_ALL, 7, desc))
        assert all(p[0].size == 7 for p in pages[:-1]) and 0 < pages[-1][0].size <= 7
        assert np.array_equal(np.concatenate([p[0] for p in pages]), whole[0]) and np.array_equal(np.concatenate([p[1] for p in pages]), whole[1])
        assert whole[2] == m.live_count()
    assert list(m.scroll(PREDS[5], 7)) == []


def test_the_model_refuses_what_the_library_refuses():
    m = handle(4)
    for kw in (dict(flags=4), dict(flags=8 | DESC), dict(limit=MAX_ORDERED + 1), dict(limit=-1)):
        with pytest.raises(ModelError):
            m.select_ordered(MATCH_ALL, kw.get("limit", 5), flags=kw.get("flags", 0))
    with pytest.raises(ModelError):
        m.select_ordered((0, 0, 0, 0, 0, 0, 2), 5)
    assert m.select_ordered(MATCH_ALL, MAX_ORDERED)[2] == m.live_count()
