"""GPU test of the one property the three searches over groups of rows share: the same row subsets expressed three ways
-- label L (vrod_search_labeled), tag bit 1 << L (vrod_search_tagged), and that tag bit with the full int64 interval
(vrod_search_where) -- answer identically, bit for bit, equal to the CPU oracle over the subset; they report the same
path and the same number of scan launches; and vrod_index_count_where reports each subset's size, however it is named.

The corpus is the smallest at which the grouping passes can go wrong: 549 rows are three blocks of the pass
(label_plan.h label_rows_per_block is 256 at this size), the last one 37 rows: a ragged wave and a partial mask word.
One label is held by 5 rows, fewer than k: its queries' lists end in unfilled slots.  PATH_GATHER sends every group
through its row list, PATH_MFMA through a masked dense scan.
"""
import numpy as np
import pytest

from support import PATH_GATHER, PATH_MFMA, ID_NONE, va, O, assert_same, oracle_over  # noqa: F401

pytestmark = pytest.mark.gpu

N, DIM, K = 549, 33, 10
LABELS = (3, 17, 62)                                 # the labels the batch asks for; L_OTHER's rows are in no subset
L_FEW, L_OTHER = 62, 9
Q_LABELS = np.array([17, 3, 62, 3, 17, 62, 3], np.uint32)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NOISE_BIT = 1 << 0                                   # a tag bit no predicate names


def test_the_shape_is_the_one_the_pass_cuts():
    """label_plan.h label_rows_per_block, restated: whole 64-row waves, at least 256 rows."""
    rpb = max(256, ((N + 2047) // 2048 + 63) // 64 * 64)
    assert rpb == 256 and -(-N // rpb) == 3 and (N - 2 * rpb) % 64 and N % 32


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(549)
    raw = rng.standard_normal((N, DIM)).astype(np.float32)
    rq = rng.standard_normal((Q_LABELS.size, DIM)).astype(np.float32)
    labels = np.array([3, 17, L_OTHER], np.uint32)[rng.integers(0, 3, N)]
    few = np.array([0, 255, 256, 511, N - 1])        # both sides of both block edges, and the last row
    labels[few] = L_FEW
    tags = (np.uint64(1) << labels.astype(np.uint64)) | (rng.integers(0, 2, N).astype(np.uint64) * np.uint64(NOISE_BIT))
    values = rng.integers(I64_MIN, I64_MAX, N, dtype=np.int64, endpoint=True)
    dead = np.setdiff1d(rng.choice(N, 24, replace=False), few)[:9].astype(np.uint64)
    return raw, rq, labels, tags, values, dead


@pytest.fixture(scope="module")
def expected(O, world):
    """Per (dtype, metric): the oracle over each query's subset, computed once."""
    raw, rq, labels, _, _, dead = world
    live = np.ones(N, bool)
    live[dead.astype(np.int64)] = False
    out = {}
    for dtype, metric in (("bf16", "cosine"), ("f32", "l2")):
        oi = np.empty((Q_LABELS.size, K), np.uint64)
        osc = np.empty((Q_LABELS.size, K), np.float32)
        for q, L in enumerate(Q_LABELS):
            oi[q], osc[q] = (x[0] for x in oracle_over(O, raw, rq[q:q + 1], K, dtype, metric, np.flatnonzero(live & (labels == L))))
        out[dtype, metric] = oi, osc
    return out


@pytest.mark.parametrize("path", [PATH_GATHER, PATH_MFMA])
@pytest.mark.parametrize("dtype,metric", [("bf16", "cosine"), ("f32", "l2")])
def test_a_subset_named_three_ways_answers_identically(va, world, expected, dtype, metric, path):
    raw, rq, labels, tags, values, dead = world
    oi, osc = expected[dtype, metric]
    bit = [1 << int(L) for L in Q_LABELS]
    with va.Index(DIM, dtype, metric) as ix:
        ix.add(raw)
        ix.set_labels(0, labels)
        ix.set_tags(0, tags)
        ix.set_values(0, values)
        ix.delete(dead)
        ix.set_path(path)
        got = {}
        for name, run in (("labeled", lambda: ix.search_labeled(rq, K, Q_LABELS)),
                          ("tagged", lambda: ix.search_tagged(rq, K, [[b, 0, 0] for b in bit])),
                          ("where", lambda: ix.search_where(rq, K, [[b, 0, 0, I64_MIN, I64_MAX] for b in bit]))):
            ids, sc = run()
            got[name] = ix.last_stats()
            assert_same(ids, sc, oi, osc, f"{name} {dtype}/{metric} path {path}")
        few = np.flatnonzero(Q_LABELS == L_FEW)
        assert (oi[few, 5:] == ID_NONE).all() and (oi[few, :5] != ID_NONE).all()     # the case has its unfilled tails
        for name in ("tagged", "where"):
            assert got[name]["path"] == got["labeled"]["path"] == path, got
            assert got[name]["scan_launches"] == got["labeled"]["scan_launches"] > 0, got
        # each subset's size, named by label, by tag bit, and by both
        live = np.ones(N, bool)
        live[dead.astype(np.int64)] = False
        want = np.array([int((live & (labels == L)).sum()) for L in LABELS], np.uint64)
        assert want[LABELS.index(L_FEW)] == 5
        for what, preds in (("label", [[0, 0, 0, I64_MIN, I64_MAX, L, 1] for L in LABELS]),
                            ("tag", [[1 << L, 0, 0, I64_MIN, I64_MAX, 0, 0] for L in LABELS]),
                            ("both", [[1 << L, 0, 0, I64_MIN, I64_MAX, L, 1] for L in LABELS])):
            assert np.array_equal(ix.count_where(preds), want), what
