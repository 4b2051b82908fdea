"""CPU tests of the near-duplicate model (near_model.py): the oracle's range scan plus a smallest-root union-find against
a brute-force restatement -- the canonical score matrix in numpy, components by repeated min-propagation -- and the
properties the device code relies on: chaining, the two trivial thresholds, and the bitwise symmetry of the score matrix
of stored rows against stored rows."""
import numpy as np
import pytest

import near_model
from near_model import ID_NONE
from support import DT, ME, O, bits, prep_of  # noqa: F401


def brute(O, rows, eligible, threshold, form, id_offset=0):
    """The same answer another way: the full score matrix, the comparison, labels that take the minimum over every edge
    until nothing changes."""
    rows = np.asarray(rows, np.float32)
    eligible = np.asarray(eligible, bool)
    count = rows.shape[0]
    s = O.numpy_scores_canonical(rows, rows, form)
    with np.errstate(invalid="ignore"):
        adj = (s >= np.float32(threshold)) if form == ME["cosine"] else (s <= np.float32(threshold))
    adj &= eligible[:, None] & eligible[None, :]
    np.fill_diagonal(adj, False)
    hits = int(adj.sum())
    adj |= adj.T
    label = np.arange(count)
    while True:
        new = np.minimum(label, np.where(adj, label[None, :], count).min(axis=1))
        if np.array_equal(new, label):
            break
        label = new
    out = np.where(eligible, label.astype(np.uint64) + np.uint64(id_offset), ID_NONE)
    el = label[eligible]
    classes = int(np.unique(el).size)
    return out, {"rows": int(eligible.sum()), "classes": classes, "near_duplicates": int(eligible.sum()) - classes,
                 "largest_class": int(np.bincount(el).max()) if el.size else 0, "hits": hits}


def clustered(n, dim, seed):
    """Unit rows: a few tight clusters, the rest singletons, shuffled."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    at = 0
    for size in (2, 3, 7, 12, 5):
        x[at + 1:at + size] = x[at] + 0.05 * rng.standard_normal((size - 1, dim)).astype(np.float32)
        at += size
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x[rng.permutation(n)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
def test_model_equals_the_brute_force_restatement(O, dtype, metric):
    raw = clustered(200, 16, 3)
    rows = O.prepare(raw, DT[dtype], prep_of(metric))
    form = ME["l2"] if metric == "l2" else ME["cosine"]
    rng = np.random.default_rng(4)
    eligible = rng.random(200) < 0.85
    s = O.numpy_scores_canonical(rows, rows, form)
    # thresholds that are scores of the set (the inclusive boundary), between tight and loose
    order = np.sort(s[np.triu_indices(200, 1)])
    picks = order[[5, 30, 200, 2000]] if form == ME["l2"] else order[[-5, -30, -200, -2000]]
    for thr in picks:
        for el, off in ((np.ones(200, bool), 0), (eligible, 7000)):
            got, gst = near_model.find_near_duplicates(O, rows, el, thr, form, off)
            want, wst = brute(O, rows, el, thr, form, off)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (thr, np.flatnonzero(got != want)[:8])
            assert gst == wst and gst["near_duplicates"] == gst["rows"] - gst["classes"], (thr, gst, wst)
            assert np.all(got[~el] == ID_NONE) and np.all(got[el] <= np.arange(200, dtype=np.uint64)[el] + np.uint64(off))
    assert wst["largest_class"] > 12                                             # the loosest threshold chains clusters together


def test_a_chain_is_one_class(O):
    """a ~ b ~ c with a and c apart: single linkage puts all three together, and the smallest row is the root."""
    t = 0.3
    rows = np.zeros((5, 4), np.float32)
    rows[4], rows[1], rows[3] = (1, 0, 0, 0), (np.cos(t), np.sin(t), 0, 0), (np.cos(2 * t), np.sin(2 * t), 0, 0)   # a = 4, b = 1, c = 3
    rows[0], rows[2] = (0, 0, 1, 0), (0, 0, 0, 1)
    s = O.numpy_scores_canonical(rows, rows, ME["cosine"])
    thr = np.float32(0.9)
    assert s[4, 1] >= thr and s[1, 3] >= thr and s[4, 3] < thr                   # the premise
    out, st = near_model.find_near_duplicates(O, rows, np.ones(5, bool), thr, ME["cosine"])
    assert out.tolist() == [0, 1, 2, 1, 1]
    assert st == {"rows": 5, "classes": 3, "near_duplicates": 2, "largest_class": 3, "hits": 4}
    d = O.numpy_scores_canonical(rows, rows, ME["l2"])
    thr = np.float32(0.2)
    assert d[4, 1] <= thr and d[1, 3] <= thr and d[4, 3] > thr
    out, st = near_model.find_near_duplicates(O, rows, np.ones(5, bool), thr, ME["l2"], id_offset=10)
    assert out.tolist() == [10, 11, 12, 11, 11] and st["hits"] == 4
    # without the middle row the ends are apart
    out, st = near_model.find_near_duplicates(O, rows, np.array([1, 0, 1, 1, 1], bool), thr, ME["l2"])
    assert out.tolist() == [0, int(ID_NONE), 2, 3, 4] and st == {"rows": 4, "classes": 4, "near_duplicates": 0, "largest_class": 1, "hits": 0}


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_the_two_trivial_thresholds(O, metric):
    rows = O.prepare(clustered(60, 8, 5), DT["f32"], prep_of(metric))
    form = ME[metric]
    none, every = (np.inf, -np.inf) if metric == "cosine" else (-np.inf, np.inf)
    out, st = near_model.find_near_duplicates(O, rows, np.ones(60, bool), none, form, 100)
    assert np.array_equal(out, np.arange(60, dtype=np.uint64) + np.uint64(100))  # nothing passes: the identity
    assert st == {"rows": 60, "classes": 60, "near_duplicates": 0, "largest_class": 1, "hits": 0}
    out, st = near_model.find_near_duplicates(O, rows, np.ones(60, bool), every, form, 100)
    assert np.all(out == np.uint64(100))                                         # everything passes: one class
    assert st == {"rows": 60, "classes": 1, "near_duplicates": 59, "largest_class": 60, "hits": 60 * 59}
    el = np.ones(60, bool)
    el[:3] = False
    out, st = near_model.find_near_duplicates(O, rows, el, every, form)
    assert np.all(out[:3] == ID_NONE) and np.all(out[3:] == np.uint64(3)) and st["hits"] == 57 * 56
    out, st = near_model.find_near_duplicates(O, rows, np.zeros(60, bool), every, form)
    assert np.all(out == ID_NONE) and st == dict.fromkeys(near_model.EXACT_STATS, 0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_stored_against_stored_scores_are_bitwise_symmetric(O, dtype, metric):
    """q*x = x*q and (q-x)^2 = (x-q)^2 element by element, summed in the same order: s[i, j] and s[j, i] are the same
    bits, so 'j qualifies for i' and 'i qualifies for j' are one statement under the canonical chains."""
    rows = O.prepare(clustered(200, 33, 6) * np.float32(3.0), DT[dtype], prep_of(metric))
    s = O.numpy_scores_canonical(rows, rows, ME[metric])
    assert np.array_equal(bits(s), bits(s.T.copy()))
    lims, ids, sc = O.scan_range(rows, rows, np.float32(np.inf if metric == "l2" else -np.inf), ME[metric])   # the C oracle's chain too
    full = np.empty((200, 200), np.float32)
    for q in range(200):
        full[q, ids[int(lims[q]):int(lims[q + 1])].astype(np.int64)] = sc[int(lims[q]):int(lims[q + 1])]
    assert np.array_equal(bits(full), bits(full.T.copy())) and np.array_equal(bits(full), bits(s))
