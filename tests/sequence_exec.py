"""Applies sequence_plans ops to the model and to a real handle side by side (test_gpu_sequence.py,
scripts/probes/sequence_fuzz.py): every mutation is followed by the counters, the labels and a few rows read back; every
check op is compared with the model in ids, score bits, NaN positions, labels and lims; every op the library must reject
has to return its status code, leave sentinel-filled buffers alone and change nothing a search can see.
"""
import ctypes as C

import numpy as np

from conftest import f32_split
from index_model import ID_NONE, ModelError, ModelIndex
from sequence_plans import PATH_AUTO, PIPE_K, PIPE_NQ, Op, _Maker, apply_mutation, every_form, expected, is_check
from support import assert_same, bits

SENT_ID, SENT_SC = np.uint64(0x5A5A5A5A5A5A5A5A), np.float32(-12345.5)
ERR_UNSUPPORTED = 6


def same_lists(got, want, what):
    assert_same(got[0], got[1], want[0], want[1], what)
    if len(want) == 3:
        assert np.array_equal(got[2], want[2]), f"{what}: labels differ at {np.argwhere(got[2] != want[2])[:5].tolist()}"


class Pair:
    """A ModelIndex and a vrod_amd.Index that are given the same ops."""

    def __init__(self, va, cfg, seed=0, devices=None):
        import torch
        self.va, self.cfg, self.seed, self.torch = va, cfg, seed, torch
        self.model = ModelIndex(cfg.dim, cfg.dtype, cfg.metric, cfg.id_offset)
        with f32_split(cfg.split):
            self.ix = va.Index(cfg.dim, cfg.dtype, cfg.metric, devices=devices)
        if cfg.id_offset:
            self.ix.set_id_offset(cfg.id_offset)
        self.rng = np.random.default_rng(seed + 1000)
        self.dev = torch.device("cuda", 0)
        # the pipelined form's buffers live as long as the handle: a graph captured in one chain is replayed in the next
        self.pq = [torch.empty((PIPE_NQ, cfg.dim), dtype=torch.float32, device=self.dev) for _ in range(2)]
        self.po = [(torch.empty((PIPE_NQ, PIPE_K), dtype=torch.int64, device=self.dev),
                    torch.empty((PIPE_NQ, PIPE_K), dtype=torch.float32, device=self.dev)) for _ in range(2)]
        self.labelled = False
        self.step = -1
        self.evens = 0
        self.gen = _Maker(seed + 2000, cfg, self.model)         # the plans' own row and query generator, over this pair's model

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ix.close()

    def where(self, op):
        return f"seed {self.seed} config {self.cfg.name} step {self.step} {op}"

    # ------------------------------------------------------------------ mutations
    def mutate(self, op):
        ix, a = self.ix, op.a
        what = self.where(op)
        if op.kind == "add":
            ix.add(a["rows"])
        elif op.kind == "delete":
            ix.delete(a["ids"])
        elif op.kind == "update":
            ix.update(a["ids"], a["rows"])
        elif op.kind == "set_filter":
            ix.set_filter(a["allow"])
        elif op.kind == "set_labels":
            ix.set_labels(a["first_id"], a["labels"])
            self.labelled = True
        elif op.kind == "set_path":
            ix.set_path(a["path"])
        got = ix.compact() if op.kind == "compact" else None
        want = apply_mutation(self.model, op)
        if op.kind == "compact":
            assert np.array_equal(got, want), f"{what}: the new-id map differs at {np.argwhere(got != want)[:5].tolist()}"
        self.state(what)

    def state(self, what):
        """The counters, the labels and three live rows read back."""
        ix, m = self.ix, self.model
        assert (ix.count, ix.live_count(), ix.filter_count()) == (m.count, m.live_count(), m.filter_count()), \
            f"{what}: count / live / eligible {(ix.count, ix.live_count(), ix.filter_count())}, the model {(m.count, m.live_count(), m.filter_count())}"
        if self.labelled and m.count:
            lab = ix.get_labels(m.offset, m.count)
            assert np.array_equal(lab, m.labels), f"{what}: labels differ at rows {np.flatnonzero(lab != m.labels)[:8].tolist()}"
        live = np.flatnonzero(~m.deleted)
        for r in self.rng.choice(live, min(3, live.size), replace=False):
            assert np.array_equal(bits(ix.get_rows(int(r), 1)), bits(m.prepared()[r:r + 1])), f"{what}: row {r} reads back differently"

    # convenience for the scripted orderings
    def add(self, rows):
        self.mutate(Op("add", dict(rows=rows)))

    def delete(self, local_rows):
        self.mutate(Op("delete", dict(ids=np.asarray(local_rows, np.uint64) + np.uint64(self.model.offset))))

    def update(self, local_rows, rows):
        self.mutate(Op("update", dict(ids=np.asarray(local_rows, np.uint64) + np.uint64(self.model.offset), rows=rows)))

    def set_filter(self, allow):
        self.mutate(Op("set_filter", dict(allow=allow)))

    def set_labels(self, first_row, labels):
        self.mutate(Op("set_labels", dict(first_id=self.model.offset + first_row, labels=np.asarray(labels, np.uint32))))

    def compact(self):
        self.mutate(Op("compact"))

    def set_path(self, path):
        self.mutate(Op("set_path", dict(path=path)))

    # ------------------------------------------------------------------ checks
    def run(self, op):
        """A check op on the handle."""
        ix, a = self.ix, op.a
        if op.kind == "search":
            return ix.search(a["rq"], a["k"])
        if op.kind == "search_labeled":
            return ix.search_labeled(a["rq"], a["k"], a["qlabels"])
        if op.kind == "search_grouped":
            return ix.search_grouped(a["rq"], a["k"])
        if op.kind == "range_search":
            return ix.range_search(a["rq"], a["thr"])
        if op.kind == "search_by_ids":
            return ix.search_by_ids(a["ids"], a["k"], a["exclude_self"])
        if op.kind == "knn_graph":
            return ix.knn_graph(a["k"], a["first_id"], a["n"])
        return self.pipeline(a["rq"], a["k"])

    def pipeline(self, rq, k):
        """A chain of pipelined searches, two in flight, over the pair's two buffer sets: every slot sees its buffers
        again and again (plain, capture, replay), whichever slot the chain starts in."""
        torch, ix = self.torch, self.ix
        assert k == PIPE_K and rq.shape[1] == PIPE_NQ
        res = []

        def begin(s):
            self.pq[s % 2].copy_(torch.from_numpy(np.ascontiguousarray(rq[s])))
            torch.cuda.synchronize()
            ix.search_begin_device(self.pq[s % 2], k, *self.po[s % 2])
        begin(0)
        for s in range(rq.shape[0]):
            if s + 1 < rq.shape[0]:
                begin(s + 1)
            ix.search_end()
            res.append((self.po[s % 2][0].cpu().numpy().view(np.uint64).copy(), self.po[s % 2][1].cpu().numpy().copy()))
        assert ix.pending == 0
        return res

    def check(self, op, tag=""):
        what = self.where(op) + (" " + tag if tag else "")
        got, want = self.run(op), expected(self.model, op)
        if op.kind == "pipelined":
            for s, (g, w) in enumerate(zip(got, want)):
                same_lists(g, w, f"{what}: search {s} of the chain")
        elif op.kind == "range_search":
            assert np.array_equal(got[0], want[0]), f"{what}: lims differ at {np.flatnonzero(got[0] != want[0])[:5].tolist()}"
            same_lists(got[1:], want[1:], what)
        else:
            same_lists(got, want, what)
        return got

    def routed(self, op, path, tag="", force=None):
        """A check op that must take the route `path`, under the handle's path as it stands or under the forced path
        `force` (the handle is back on AUTO afterwards) -> the counters of that search."""
        if force is not None:
            self.ix.set_path(force)
        try:
            self.check(op, tag)
            st = self.ix.last_stats()
        finally:
            if force is not None:
                self.ix.set_path(PATH_AUTO)
        assert st["path"] == path, f"{self.where(op)} {tag}: took path {st['path']}, not {path}: {st}"
        return st

    def read_back(self, local_rows, what):
        """Whole rows read back, live or deleted: the bits of the model's prepared rows."""
        pc = self.model.prepared()
        rows = np.unique(np.asarray(local_rows, np.int64))
        for run in np.split(rows, np.flatnonzero(np.diff(rows) > 1) + 1):       # a call per stretch of neighbouring rows
            lo, n = int(run[0]), int(run.size)
            got, want = bits(self.ix.get_rows(lo, n)), bits(pc[lo:lo + n])
            assert np.array_equal(got, want), f"{what}: rows {(lo + np.flatnonzero((got != want).any(axis=1)))[:8].tolist()} read back differently"

    def fresh_rows(self, n):
        return self.gen.rows(n)

    def queries(self, nq):
        return self.gen.queries(nq)

    def rank_thresholds(self, rq, rank):
        """Per query the model's rank-th best score over the eligible rows: a range search at it returns that row too."""
        return self.model.search(rq, rank)[1][:, rank - 1].copy()

    def check_every_form(self, tag, nqs=(3, 40), k=10, forms=None):
        self.evens += 1
        for op in every_form(self.seed * 1000 + self.evens, self.cfg, self.model, nqs, k):
            if forms is None or op.kind in forms:
                self.check(op, tag)

    # ------------------------------------------------------------------ ops the library must reject
    def raises(self, code, call, what):
        try:
            call()
        except self.va.VrodError as e:
            assert e.code == code, f"{what}: status {e.code}, documented {code}"
        else:
            raise AssertionError(f"{what}: the call was accepted")

    def reject(self, op):
        ix, m, a = self.ix, self.model, op.a
        what, w, code = self.where(op), op.a["what"], op.a["code"]
        if w == "add_nan":
            self.raises(code, lambda: ix.add(a["rows"]), what)
            try:
                m.add(a["rows"])
            except ModelError:
                pass
        elif w in ("update_nan", "update_deleted"):
            self.raises(code, lambda: ix.update(a["ids"], a["rows"]), what)
        elif w == "byid_deleted":
            ids = np.ascontiguousarray(a["ids"], np.uint64)
            oi = np.full((ids.size, a["k"]), SENT_ID, np.uint64)
            sc = np.full((ids.size, a["k"]), SENT_SC, np.float32)
            rc = ix._L.vrod_search_by_ids(ix._h, ids.ctypes.data_as(C.c_void_p), ids.size, a["k"], int(a["exclude_self"]),
                                          oi.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p))
            assert rc == code and (oi == SENT_ID).all() and (sc == SENT_SC).all(), f"{what}: status {rc}, or the outputs were written"
        elif w == "compact_map_len":
            buf = np.full(max(a["map_len"], m.count) + 1, SENT_ID, np.uint64)
            rc = ix._L.vrod_index_compact(ix._h, buf.ctypes.data_as(C.c_void_p), int(a["map_len"]))
            assert rc == code and (buf == SENT_ID).all(), f"{what}: status {rc}, or the map was written"
        else:                                          # a mutation while a search is pending
            torch, inner = self.torch, a["op"]
            self.pq[0].copy_(torch.from_numpy(np.ascontiguousarray(a["rq"])))
            torch.cuda.synchronize()
            ix.search_begin_device(self.pq[0], PIPE_K, *self.po[0])
            call = {"add": lambda: ix.add(inner.a["rows"]), "delete": lambda: ix.delete(inner.a["ids"]),
                    "update": lambda: ix.update(inner.a["ids"], inner.a["rows"]), "set_filter": lambda: ix.set_filter(inner.a["allow"]),
                    "set_labels": lambda: ix.set_labels(inner.a["first_id"], inner.a["labels"]), "compact": ix.compact}[inner.kind]
            try:
                self.raises(code, call, what)
                assert ix.pending == 1, what
            finally:
                ix.search_end()
            got = (self.po[0][0].cpu().numpy().view(np.uint64), self.po[0][1].cpu().numpy())
            same_lists(got, m.search(a["rq"], PIPE_K), f"{what}: the pending search itself")
        self.state(what)
        same_lists(ix.search(a["after_rq"], 10), m.search(a["after_rq"], 10), f"{what}: the search right after")

    # ------------------------------------------------------------------ a whole plan
    def run_plan(self, plan):
        for self.step, op in enumerate(plan):
            if op.kind == "reject":
                self.reject(op)
            elif is_check(op):
                self.check(op)
            else:
                self.mutate(op)
        self.step = len(plan)
        self.check_every_form("at the end of the plan", nqs=(9,))
