"""GPU test of a handle that keeps all four row columns (labels, tags, values, keys), tombstones and a filter alive at
once, across the paths that keep those arrays in step with the corpus: growth (twice, the second from a grown state),
compaction, save / load, and the growth of a handle whose columns came from a snapshot.

What the handle should hold is plain numpy (class State).  After every step:
  - the host mirrors: get_labels / get_tags / get_values / get_keys over [0, count) equal the expected arrays;
  - the device copies, which the getters never read, through the device: search_labeled with one label per query,
    search_tagged with any-of masks and search_where with value intervals.  Every predicate used is matched by at most 40
    eligible rows of the expected state (asserted), fewer than k = 64, so the returned ids, ID_NONE dropped, must be
    exactly the numpy set of eligible matching rows whatever the scores are; find_keys_device over every key plus three
    absent ones and ids_to_keys_device over [0, count + 2);
  - filter_count() and live_count(), and a plain search with the five newest rows as queries: it returns eligible rows
    only, so none of those five once the filter is set (the filter's last five rows are not allowed, later rows never are).

Sizes: dim 8; 300 rows (capacity 512), + 400 (768), + 700 (1536), compacted, saved, loaded (capacity 1536 again: the rows
left are more than 1280), + 300 (a growth of the loaded handle).  Integers and id sets: every comparison is exact.
"""
import numpy as np
import pytest

from support import ID_NONE, va  # noqa: F401

pytestmark = pytest.mark.gpu

DIM, K, MOST = 8, 64, 40
CONFIGS = (("f32", "cosine"), ("bf16", "l2"))
ABSENT = np.array([5, 10**12, 2**63 - 1], np.uint64)              # keys no row is ever given


class State:
    """The rows' columns, tombstones and allowed bits as the handle should hold them."""

    def __init__(self):
        self.rows = np.zeros((0, DIM), np.float32)
        self.labels = np.zeros(0, np.uint32)
        self.tags = np.zeros(0, np.uint64)
        self.values = np.zeros(0, np.int64)
        self.keys = np.zeros(0, np.uint64)
        self.dead = np.zeros(0, bool)
        self.allow = None                                          # no filter yet

    @property
    def count(self):
        return len(self.rows)

    def add(self, rows):
        n = len(rows)
        self.rows = np.concatenate([self.rows, rows])
        self.labels = np.concatenate([self.labels, np.zeros(n, np.uint32)])
        self.tags = np.concatenate([self.tags, np.zeros(n, np.uint64)])
        self.values = np.concatenate([self.values, np.zeros(n, np.int64)])
        self.keys = np.concatenate([self.keys, np.full(n, ID_NONE)])
        self.dead = np.concatenate([self.dead, np.zeros(n, bool)])
        if self.allow is not None:
            self.allow = np.concatenate([self.allow, np.zeros(n, bool)])      # rows added later are not allowed

    def compact(self):
        keep = ~self.dead
        for name in ("rows", "labels", "tags", "values", "keys", "allow", "dead"):
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name)[keep])

    def eligible(self):
        return ~self.dead if self.allow is None else ~self.dead & self.allow


def id_set(row):
    return set(int(i) for i in row[row != ID_NONE])


def narrow(S, masks, what, expect_some):
    """The predicates (by index) that at most MOST eligible rows match, with the rows of each."""
    elig = S.eligible()
    kept = [(j, np.flatnonzero(elig & m)) for j, m in enumerate(masks)]
    kept = [(j, rows) for j, rows in kept if rows.size <= MOST]
    assert all(rows.size <= MOST < K for _, rows in kept), what
    if expect_some:                                                # the columns are set: the check is not about empty sets only
        assert sum(rows.size > 0 for _, rows in kept) >= 3, what
    return kept


def check(ix, S, queries, what, columns_set=True):
    import torch
    n = S.count
    assert ix.count == n, what
    # the host mirrors
    assert np.array_equal(ix.get_labels(0, n), S.labels), what
    assert np.array_equal(ix.get_tags(0, n), S.tags), what
    assert np.array_equal(ix.get_values(0, n), S.values), what
    assert np.array_equal(ix.get_keys(0, n), S.keys), what
    # filter and liveness
    elig = S.eligible()
    assert ix.live_count() == int((~S.dead).sum()) and ix.filter_count() == int(elig.sum()), what
    # the device copies of labels, tags and values, through the searches that read them
    labs = np.array(list(range(0, 14)) + [99], np.uint32)
    kept = narrow(S, [S.labels == l for l in labs], what, columns_set)
    ids, _ = ix.search_labeled(queries[:len(kept)], K, labs[[j for j, _ in kept]])
    for q, (j, rows) in enumerate(kept):
        assert id_set(ids[q]) == set(rows.tolist()), (what, "label", int(labs[j]))
    anys = np.array([1, 2, 4, 8, 16, 32, 3, 40, 64], np.uint64)
    kept = narrow(S, [(S.tags & a) != 0 for a in anys], what, columns_set)
    preds = np.zeros((len(kept), 3), np.uint64)
    preds[:, 0] = anys[[j for j, _ in kept]]
    ids, _ = ix.search_tagged(queries[:len(kept)], K, preds)
    for q, (j, rows) in enumerate(kept):
        assert id_set(ids[q]) == set(rows.tolist()), (what, "any-of", int(anys[j]))
    spans = [(-20, -18), (-12, -10), (-1, 1), (5, 5), (7, 9), (18, 20), (21, 30)]
    kept = narrow(S, [(S.values >= lo) & (S.values <= hi) for lo, hi in spans], what, columns_set)
    ids, _ = ix.search_where(queries[:len(kept)], K, [[0, 0, 0, *spans[j]] for j, _ in kept])
    for q, (j, rows) in enumerate(kept):
        assert id_set(ids[q]) == set(rows.tolist()), (what, "interval", spans[j])
    # the device copy of the keys and the table
    asked = np.concatenate([S.keys[S.keys != ID_NONE], ABSENT])
    holder = {int(key): r for r, key in enumerate(S.keys) if key != ID_NONE and not S.dead[r]}
    want = np.array([holder.get(int(key), int(ID_NONE)) for key in asked], np.uint64)
    got = ix.find_keys_device(torch.from_numpy(asked.view(np.int64)).cuda())
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want), what
    d_ids = torch.arange(n + 2, dtype=torch.int64, device="cuda")
    want = np.concatenate([S.keys, np.full(2, ID_NONE)])
    assert np.array_equal(ix.ids_to_keys_device(d_ids).cpu().numpy().view(np.uint64), want), what
    # a plain search with the newest rows as queries
    ids, _ = ix.search(S.rows[n - 5:], K)
    assert id_set(ids.reshape(-1)) <= set(np.flatnonzero(elig).tolist()), what
    if S.allow is not None:
        assert not elig[n - 5:].any() and not id_set(ids.reshape(-1)) & set(range(n - 5, n)), what


@pytest.mark.parametrize("dtype,metric", CONFIGS)
def test_columns_tombstones_and_filter_together(va, tmp_path, dtype, metric):
    rng = np.random.default_rng(5150)
    raw = rng.standard_normal((300 + 400 + 700 + 300, DIM)).astype(np.float32)
    queries = rng.standard_normal((16, DIM)).astype(np.float32)
    S = State()
    ix = va.Index(DIM, dtype, metric)
    try:
        def add(lo, hi):
            ix.add(raw[lo:hi])
            S.add(raw[lo:hi])

        add(0, 300)                                                # capacity 512
        check(ix, S, queries, "300 rows, nothing set", columns_set=False)

        S.labels[:] = rng.integers(1, 13, 300)                     # 12 distinct labels, none of them the default
        S.tags[:] = (rng.random((300, 6)) < 0.08) @ (1 << np.arange(6))      # 6 tag bits, sparse
        S.values[:] = rng.integers(-20, 21, 300)
        S.keys[:] = 1000 + 7 * rng.permutation(300).astype(np.uint64)
        ix.set_labels(0, S.labels)
        ix.set_tags(0, S.tags)
        ix.set_values(0, S.values)
        ix.set_keys(0, S.keys)
        check(ix, S, queries, "columns set")

        dead = rng.choice(295, 30, replace=False)
        ix.delete(dead)
        S.dead[dead] = True
        check(ix, S, queries, "30 rows deleted")

        S.allow = rng.random(300) < 0.5
        S.allow[295:] = False
        ix.set_filter(S.allow)
        check(ix, S, queries, "filter set")

        add(300, 700)                                              # capacity 768
        check(ix, S, queries, "grown once")
        add(700, 1400)                                             # capacity 1536, from a state that has grown already
        check(ix, S, queries, "grown twice")

        new_ids = ix.compact()
        assert np.array_equal(new_ids[~S.dead], np.arange(1370, dtype=np.uint64)) and (new_ids[S.dead] == ID_NONE).all()
        S.compact()
        check(ix, S, queries, "compacted")
        assert ix.key_stats()["keyed_live"] == int((S.keys != ID_NONE).sum()) == 270

        first, again = tmp_path / "first.vrod", tmp_path / "again.vrod"
        ix.save(first)
        with va.Index.load(first) as loaded:
            check(loaded, S, queries, "loaded")
            assert loaded.key_stats()["keyed_live"] == 270
            loaded.save(again)
            assert first.read_bytes() == again.read_bytes()
            loaded.add(raw[1400:])                                 # a growth of columns that came from the snapshot
            S.add(raw[1400:])
            check(loaded, S, queries, "loaded, then grown")
    finally:
        ix.close()
