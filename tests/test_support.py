"""The shared test helpers (support.py) are what every feature test's verdict rests on: tested here, on the CPU.

  - assert_same must refuse every kind of difference a result can show, and accept NaN filler in equal slots;
  - oracle_over + eligible_rows must give what index_model.ModelIndex expects of a search (two independent routes to the
    same quantity: the oracle over the eligible rows, positions mapped back to ids + offset);
  - takes_segments must equal the real filter_route of search_plan.h, over the table test_filter_plan.py's host driver
    prints;
  - row_bytes must follow the padding rule of the stored rows.
"""
import numpy as np
import pytest

from index_model import ModelIndex
from support import DT, ID_NONE, assert_same, assert_same_all_bits, bits, eligible_rows, oracle_over, row_bytes, takes_segments
from test_filter_plan import table  # noqa: F401  (the compiled driver around the real filter_route)


# ---------------------------------------------------------------- assert_same
def lists():
    ids = np.arange(12, dtype=np.uint64).reshape(3, 4)
    sc = np.linspace(0.5, 1.5, 12, dtype=np.float32).reshape(3, 4)
    ids[1, 3], sc[1, 3] = ID_NONE, np.nan
    ids[2, 2:], sc[2, 2:] = ID_NONE, np.nan
    sc[0, 0] = 0.0
    return ids, sc


def test_assert_same_accepts_equal_lists_with_nans_in_equal_slots():
    ids, sc = lists()
    assert_same(ids, sc, ids.copy(), sc.copy(), "equal")
    assert_same(ids[:0], sc[:0], ids[:0].copy(), sc[:0].copy(), "empty")


def one_id(ids, sc):
    ids[0, 1] += np.uint64(1)


def nan_moved(ids, sc):
    sc[1, 2], sc[1, 3] = sc[1, 3], sc[1, 2]


def one_ulp(ids, sc):
    sc[2, 1] = np.nextafter(sc[2, 1], np.float32(2))


def signed_zero(ids, sc):
    sc[0, 0] = -0.0


@pytest.mark.parametrize("change", [one_id, nan_moved, one_ulp, signed_zero])
def test_assert_same_refuses(change):
    ids, sc = lists()
    oi, osc = ids.copy(), sc.copy()
    change(oi, osc)
    for check in (assert_same, assert_same_all_bits):
        with pytest.raises(AssertionError, match="differ"):
            check(ids, sc, oi, osc, change.__name__)
        with pytest.raises(AssertionError, match="differ"):
            check(oi, osc, ids, sc, change.__name__)


@pytest.mark.parametrize("cut", [(slice(None), slice(0, 3)), (slice(0, 2), slice(None))], ids=["columns", "rows"])
@pytest.mark.parametrize("which", ["ids", "scores", "both"])
def test_assert_same_refuses_a_shape_mismatch(cut, which):
    ids, sc = lists()
    oi = ids[cut] if which != "scores" else ids
    osc = sc[cut] if which != "ids" else sc
    with pytest.raises(AssertionError, match="shapes differ"):
        assert_same(ids, sc, oi, osc, "shape")
    # ... also where broadcasting would have made the values compare equal
    one = np.zeros((1, 4), np.uint64), np.ones((1, 4), np.float32)
    three = np.zeros((3, 4), np.uint64), np.ones((3, 4), np.float32)
    with pytest.raises(AssertionError, match="shapes differ"):
        assert_same(*three, *one, "broadcast")


def test_all_bits_form_also_compares_nan_payloads():
    ids, sc = lists()
    osc = sc.copy()
    osc.view(np.uint32)[1, 3] ^= np.uint32(1)       # still a NaN, another payload
    assert np.isnan(osc[1, 3])
    assert_same(ids, sc, ids, osc, "payload")
    with pytest.raises(AssertionError, match="score bits differ"):
        assert_same_all_bits(ids, sc, ids, osc, "payload")


# ---------------------------------------------------------------- oracle_over + eligible_rows against the model
N, DIM, NQ, OFFSET = 300, 8, 5, 10 ** 9 + 7


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(31)
    raw = rng.standard_normal((N, DIM)).astype(np.float32)
    raw[17] = raw[16]                                # a tie: the smaller id first on both routes
    raw *= np.exp(rng.uniform(-1.0, 1.0, (N, 1))).astype(np.float32)
    rq = rng.standard_normal((NQ, DIM)).astype(np.float32)
    deleted = np.unique(rng.choice(N, 40, replace=False))
    allow = rng.random(220) < 0.6                    # shorter than the count: rows 220 .. 299 are not allowed
    return raw, rq, deleted, allow


def model_of(raw, dtype, metric, deleted=(), allow=None):
    m = ModelIndex(DIM, dtype, metric, OFFSET)
    m.add(raw)
    m.delete(np.asarray(deleted, dtype=np.uint64) + np.uint64(OFFSET))
    m.set_filter(allow)
    return m


@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", sorted(DT))
def test_oracle_over_equals_the_model(oracle, corpus, dtype, metric):
    raw, rq, deleted, allow = corpus
    for what, dele, alw in (("deleted + allow", deleted, allow), ("deleted", deleted, None), ("allow", (), allow), ("all rows", (), None)):
        el = eligible_rows(N, alw, dele)
        want = np.ones(N, bool)
        if alw is not None:
            want[:] = False
            want[:alw.size] = alw
        want[np.asarray(dele, dtype=np.int64)] = False
        assert np.array_equal(el, np.flatnonzero(want)), what
        m = model_of(raw, dtype, metric, dele, alw)
        assert m.filter_count() == el.size
        for k in (1, 10, el.size, el.size + 7):      # the last: more than the eligible rows, (ID_NONE, NaN) past them
            ids, sc = oracle_over(oracle, raw, rq, k, dtype, metric, el, OFFSET)
            assert ids.dtype == np.uint64 and sc.dtype == np.float32 and ids.shape == (NQ, k)
            assert_same_all_bits(ids, sc, *m.search(rq, k), f"{what} k={k}")
            filler = max(0, k - el.size)
            assert (ids[:, k - filler:] == ID_NONE).all() and np.isnan(sc[:, k - filler:]).all(), (what, k)
            assert (ids[:, :k - filler] >= np.uint64(OFFSET)).all() and not np.isnan(sc[:, :k - filler]).any(), (what, k)


@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", sorted(DT))
def test_oracle_over_no_eligible_row(oracle, corpus, dtype, metric):
    raw, rq, _, _ = corpus
    for el in (eligible_rows(N, np.zeros(0, bool)), eligible_rows(N, None, np.arange(N)), eligible_rows(N, np.zeros(N, bool))):
        assert el.size == 0
        ids, sc = oracle_over(oracle, raw, rq, 6, dtype, metric, el, OFFSET)
        assert ids.shape == sc.shape == (NQ, 6) and ids.dtype == np.uint64 and sc.dtype == np.float32
        assert (ids == ID_NONE).all() and np.isnan(sc).all()
    assert_same(ids, sc, *model_of(raw, dtype, metric, np.arange(N)).search(rq, 6), "model, every row deleted")


# ---------------------------------------------------------------- takes_segments against search_plan.h
def test_takes_segments_is_the_headers_filter_route(table):  # noqa: F811
    wrong = [(key, g) for key, g in table.items()
             if takes_segments(key[1], ("f32", "bf16")[key[0]], key[2], key[5], key[4], key[3]) != g]
    assert len(table) > 100_000
    assert not wrong, f"{len(wrong)} of {len(table)} decisions differ, first {wrong[:5]} (dtype, forced, N, dim, nq, m)"


# ---------------------------------------------------------------- row_bytes
@pytest.mark.parametrize("dim", [1, 31, 32, 33, 63, 64, 65])
def test_row_bytes_follows_the_padding_rule(dim):
    # a stored row is padded to whole 128-byte chunks: 64 bf16 values, 32 fp32 values
    chunks_bf16 = {1: 1, 31: 1, 32: 1, 33: 1, 63: 1, 64: 1, 65: 2}[dim]
    chunks_f32 = {1: 1, 31: 1, 32: 1, 33: 2, 63: 2, 64: 2, 65: 3}[dim]
    assert row_bytes("bf16", dim) == 128 * chunks_bf16
    assert row_bytes("f32", dim) == 128 * chunks_f32
    for dtype, size in (("bf16", 2), ("f32", 4)):
        assert row_bytes(dtype, dim) % 128 == 0 and 0 <= row_bytes(dtype, dim) - dim * size < 128


def test_bits_keeps_the_sign_of_zero_and_nan_payloads():
    assert bits(np.float32(0.0)) != bits(np.float32(-0.0))
    assert bits(np.array([np.nan], np.float32))[0] == 0x7FC00000
