"""A plain-Python model of one vrod_index handle: what a long-lived handle must hold after any order of operations.

numpy plus the CPU oracle; no GPU and no import of the library.  The model keeps the RAW fp32 rows, a `deleted` array,
the allow list (None or bools), the labels and the id offset, and mirrors the documented semantics of include/vrod.h:
  add         new rows are live, carry label 0 and are not allowed while a filter is set
  delete      all or nothing; naming a row twice, or a deleted row, is fine
  update      all or nothing; an id named twice takes the last vector; a deleted or unknown id rejects the call
  set_filter  an array shorter than the count is fine, rows past it are not allowed; None clears
  set_labels  a range of ids; deleted rows may be named
  compact     rows, labels and allowed bits move with their rows, the tombstones are cleared; returns the new-id map
A call the library must reject raises ModelError with the documented status code and changes nothing -- except the
capacity, which index_add grows before it looks at the values (the model tracks the capacity by index_reserve's rule only
so that sequence_plans.coverage() can count the growths).

Expected results of EVERY search form come from one primitive: oracle.prepare of the current rows (cached, redone for
the rows a mutation touched), then oracle.scan_topk / oracle.scan_range over the eligible (live and allowed) rows taken in
ascending order, positions mapped back to ids + offset.

The codes (DT, the metric codes, ID_NONE), THREADS and the helpers bits and drop_self come from support.py, the bottom
layer of the test helpers; this module defines the model and its status codes only.
"""
import numpy as np

from oracle import oracle as O

from support import DT, ID_NONE, METRIC_COSINE, METRIC_L2, THREADS, drop_self

ERR_INVALID_ARG, ERR_INVALID_VALUE, ERR_UNSUPPORTED = 1, 2, 6
ROW_TILE = 256                                     # index_reserve rounds the capacity up to this


class ModelError(Exception):
    def __init__(self, code, what=""):
        super().__init__(f"status {code}: {what}")
        self.code = code


class ModelIndex:
    def __init__(self, dim, dtype, metric, id_offset=0):
        self.dim, self.dtype, self.metric = int(dim), dtype, metric
        self.offset = int(id_offset)
        self.prep = METRIC_COSINE if metric == "cosine" else METRIC_L2      # how rows and queries are prepared
        self.form = METRIC_L2 if metric == "l2" else METRIC_COSINE          # how a pair is scored
        self.rows = np.zeros((0, self.dim), np.float32)
        self.deleted = np.zeros(0, bool)
        self.allow = None
        self.labels = np.zeros(0, np.uint32)
        self.capacity = 0
        self._pc = np.zeros((0, self.dim), np.float32)

    # ------------------------------------------------------------------ counters
    @property
    def count(self):
        return self.rows.shape[0]

    def live_count(self):
        return int((~self.deleted).sum())

    def eligible(self):
        return ~self.deleted if self.allow is None else ~self.deleted & self.allow

    def filter_count(self):
        return int(self.eligible().sum())

    # ------------------------------------------------------------------ mutations
    def _prepare(self, raw):
        return O.prepare(raw, DT[self.dtype], self.prep, threads=THREADS)

    def prepared(self):
        """oracle.prepare of the current rows (what get_rows reads back)."""
        return self._pc

    def _local(self, ids, what):
        ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
        with np.errstate(over="ignore"):
            loc = ids - np.uint64(self.offset)
        if ((ids < np.uint64(self.offset)) | (loc >= np.uint64(self.count))).any():
            raise ModelError(ERR_INVALID_ARG, f"{what}: an id that is no current row")
        return loc.astype(np.int64)

    def add(self, raw):
        """-> True if the capacity grew."""
        raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, self.dim)
        n = raw.shape[0]
        if n == 0:
            return False
        grew = False
        if self.count + n > self.capacity:           # index_add, index_reserve
            want = max(self.count + n, self.capacity + self.capacity // 2) if self.capacity else self.count + n
            self.capacity = -(-max(want, 1) // ROW_TILE) * ROW_TILE
            grew = True
        if not np.isfinite(raw).all():
            raise ModelError(ERR_INVALID_VALUE, "add: NaN or Inf")
        self.rows = np.concatenate([self.rows, raw])
        self._pc = np.concatenate([self._pc, self._prepare(raw)])
        self.deleted = np.concatenate([self.deleted, np.zeros(n, bool)])
        self.labels = np.concatenate([self.labels, np.zeros(n, np.uint32)])
        if self.allow is not None:
            self.allow = np.concatenate([self.allow, np.zeros(n, bool)])
        return grew

    def delete(self, ids):
        loc = self._local(ids, "delete")
        self.deleted = self.deleted.copy()
        self.deleted[loc] = True

    def update(self, ids, raw):
        raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, self.dim)
        loc = self._local(ids, "update")
        if self.deleted[loc].any():
            raise ModelError(ERR_INVALID_ARG, "update: a deleted row")
        if not np.isfinite(raw).all():
            raise ModelError(ERR_INVALID_VALUE, "update: NaN or Inf")
        if loc.size == 0:
            return
        self.rows = self.rows.copy()
        self._pc = self._pc.copy()
        pr = self._prepare(raw)
        for i, r in enumerate(loc):                  # in order: the last vector of a repeated id stays
            self.rows[r], self._pc[r] = raw[i], pr[i]

    def set_filter(self, allow):
        if allow is None:
            self.allow = None
            return
        a = np.asarray(allow, dtype=bool).reshape(-1)
        if a.size > self.count:
            raise ModelError(ERR_INVALID_ARG, "set_filter: more entries than rows")
        full = np.zeros(self.count, bool)
        full[:a.size] = a
        self.allow = full

    def set_labels(self, first_id, labels):
        labels = np.asarray(labels, dtype=np.uint32).reshape(-1)
        if labels.size == 0:
            return
        first = int(first_id) - self.offset
        if first < 0 or first + labels.size > self.count:
            raise ModelError(ERR_INVALID_ARG, "set_labels: a range past the rows")
        self.labels = self.labels.copy()
        self.labels[first:first + labels.size] = labels

    def compact(self, map_len=None):
        if map_len is not None and map_len != self.count:
            raise ModelError(ERR_INVALID_ARG, "compact: map_len is not the count")
        keep = ~self.deleted
        new_ids = np.full(self.count, ID_NONE, np.uint64)
        new_ids[keep] = np.arange(int(keep.sum()), dtype=np.uint64) + np.uint64(self.offset)
        if not keep.all():
            self.rows, self._pc, self.labels = self.rows[keep], np.ascontiguousarray(self._pc[keep]), self.labels[keep]
            if self.allow is not None:
                self.allow = self.allow[keep]
            self.deleted = np.zeros(self.rows.shape[0], bool)
        return new_ids

    # ------------------------------------------------------------------ the one primitive
    def _topk(self, rows, pq, k):
        """The oracle's top-k of prepared queries over the prepared rows `rows` (ascending local rows) -> (ids, scores)."""
        nq = pq.shape[0]
        if rows.size == 0 or nq == 0:
            return np.full((nq, k), ID_NONE, np.uint64), np.full((nq, k), np.nan, np.float32)
        i, s = O.scan_topk(np.ascontiguousarray(self._pc[rows]), pq, k, self.form, threads=THREADS)
        none = i == ID_NONE
        at = np.where(none, 0, i).astype(np.int64)
        return np.where(none, ID_NONE, rows[at].astype(np.uint64) + np.uint64(self.offset)), s

    def _queries(self, rq):
        rq = np.ascontiguousarray(rq, dtype=np.float32).reshape(-1, self.dim)
        return self._prepare(rq)

    # ------------------------------------------------------------------ the search forms
    def search(self, rq, k):
        return self._topk(np.flatnonzero(self.eligible()), self._queries(rq), k)

    def search_labeled(self, rq, k, qlabels):
        pq = self._queries(rq)
        qlabels = np.asarray(qlabels, dtype=np.uint32).reshape(-1)
        ids = np.full((pq.shape[0], k), ID_NONE, np.uint64)
        sc = np.full((pq.shape[0], k), np.nan, np.float32)
        elig = self.eligible()
        for L in np.unique(qlabels):
            qs = np.flatnonzero(qlabels == L)
            ids[qs], sc[qs] = self._topk(np.flatnonzero(elig & (self.labels == L)), np.ascontiguousarray(pq[qs]), k)
        return ids, sc

    def search_grouped(self, rq, k):
        pq = self._queries(rq)
        nq = pq.shape[0]
        elig = self.eligible()
        present = np.unique(self.labels[elig])
        ids = np.empty((nq, present.size), np.uint64)
        sc = np.empty((nq, present.size), np.float32)
        for j, L in enumerate(present):              # every label's representative: the oracle's top-1 over its rows
            i, s = self._topk(np.flatnonzero(elig & (self.labels == L)), pq, 1)
            ids[:, j], sc[:, j] = i[:, 0], s[:, 0]
        lab = np.broadcast_to(present.astype(np.uint32), ids.shape).copy()
        oi = np.full((nq, k), ID_NONE, np.uint64)
        osc = np.full((nq, k), np.nan, np.float32)
        ol = np.zeros((nq, k), np.uint32)
        m = min(k, present.size)
        for q in range(nq):
            nan = np.isnan(sc[q])
            val = np.where(nan, np.float32(0), sc[q] if self.form == METRIC_L2 else -sc[q])
            o = np.lexsort((ids[q], val, nan))[:m]   # NaN last, then the score, then the id
            oi[q, :m], osc[q, :m], ol[q, :m] = ids[q][o], sc[q][o], lab[q][o]
        return oi, osc, ol

    def range_search(self, rq, thr):
        pq = self._queries(rq)
        rows = np.flatnonzero(self.eligible())
        if rows.size == 0 or pq.shape[0] == 0:
            return np.zeros(pq.shape[0] + 1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.float32)
        lims, pos, sc = O.scan_range(np.ascontiguousarray(self._pc[rows]), pq, thr, self.form, threads=THREADS)
        return lims, rows[pos.astype(np.int64)].astype(np.uint64) + np.uint64(self.offset), sc

    def search_by_ids(self, ids, k, exclude_self=False):
        loc = self._local(ids, "search_by_ids")
        if self.deleted[loc].any():
            raise ModelError(ERR_INVALID_ARG, "search_by_ids: a deleted row")
        pq = np.ascontiguousarray(self._pc[loc])     # the prepared stored rows, as they are
        rows = np.flatnonzero(self.eligible())
        if not exclude_self:
            return self._topk(rows, pq, k)
        i, s = self._topk(rows, pq, k + 1)
        return drop_self(i, s, loc.astype(np.uint64) + np.uint64(self.offset), k)

    def knn_graph(self, k, first_id=None, n=None):
        first = 0 if first_id is None else int(first_id) - self.offset
        n = self.count - first if n is None else int(n)
        if first < 0 or first + n > self.count:
            raise ModelError(ERR_INVALID_ARG, "knn_graph: a range past the rows")
        ids = np.full((n, k), ID_NONE, np.uint64)
        sc = np.full((n, k), np.nan, np.float32)
        live = first + np.flatnonzero(~self.deleted[first:first + n])
        if live.size:
            ids[live - first], sc[live - first] = self.search_by_ids(live.astype(np.uint64) + np.uint64(self.offset), k, True)
        return ids, sc
