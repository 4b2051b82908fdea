"""Deterministic plans of operations on one handle, made against the model alone (index_model.ModelIndex).

make_plan(seed, config) -> list[Op].  A plan starts from an empty handle without reserve() and runs 40 or 41 steps:
mutations (add, delete, update, set_filter, set_labels, compact, set_path), ops the library must reject, and check ops that
name one search form and its shape.  Nothing here touches a handle: test_gpu_sequence.py applies every op to the model and
to a real handle, test_sequence_plans.py replays the plans on the model to count what they reach (coverage()).

The backbone of a plan is fixed so that every plan reaches the orderings the per-feature tests never scripted, and the
random generator fills in sizes, ids, shapes and the order inside each phase:
  A  add 1500, add 300 (the first growth), then in any order: the labelling, a delete, a broad or short filter
  B  in any order: the gather / labelled / gather triple, then the path AUTO or MFMA; on one of those (the routes that
     build the planes of an f32 handle) a batched search, an add within the capacity, an update on both sides of the old
     count, a batched search; a rejected op.  Then two adds that each outgrow the capacity while tombstones, a filter and
     labels exist, a rejected op between them
  H  with the path STREAM (the route search_enqueue captures and replays whatever the filter's density) the pipelined
     search -- buffers kept for the whole plan, so a graph captured in one chain is replayed in the next -- before and
     after two of the labelled, grouped, range and by-id searches (which two rotates with the seed)
  C  a change of path (half of the plans), a delete of a stretch, a compaction under the filter and the labels, an add
     after it, a mutation while a search is pending, a cleared filter (the other half) and then a narrow filter with a k
     above the eligible rows
After every mutation comes a check whose form rotates with the seed, so that the committed seeds together put every search
form behind every kind of mutation.

Where the plans leave the issue's figures, and why.  The issue asks for totals of 1 500 .. 8 000 rows, a labelling with
about 40 labels of about 20 rows beside a label on more than half of the rows (so at least 1 800 rows), two capacity growths
under tombstones, filter and labels, and a model-against-numpy check on plans of at most 2 000 rows: two growths from 1 800
rows end above 3 400.  So COMMITTED holds eight full-size plans that meet all of it and run on the GPU, and MODEL_CHECK three
`small` plans of the same backbone at 337 .. 1 300 rows (about 7 small labels) that exist for the CPU check of the model
alone.  An f32 handle with VROD_F32_SPLIT=0 never has planes, so counter (d) is asked of the other f32 plans only.

coverage() routes a search the way the library does (route and graph_route of search_plan.h, restated
below; filter_route is support.takes_segments): an ordering counts only if the search in it takes the route the ordering is
about.
"""
from dataclasses import dataclass, field

import numpy as np

from index_model import ModelError, ModelIndex
from support import PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER, takes_segments as filter_route

MUTATIONS = ("add", "delete", "update", "set_filter", "set_labels", "compact", "set_path")
FORMS = ("search", "search_labeled", "search_grouped", "range_search", "search_by_ids", "knn_graph", "pipelined")
ADD_SIZES = (1, 37, 300, 1500)
NQS = (1, 3, 9, 40, 300)
KS = (1, 10, 50)
L_BIG, L_SMALL0, L_NOBODY = 3_000_000_000, 1000, 77       # the label of most rows, the first small label, a label no row has
N_SMALL, SMALL_ROWS = 40, 20
KNN_MAX_ROWS, KNN_PER_PLAN = 3000, 2
PIPE_NQ, PIPE_K, PIPE_CHAIN = 3, 10, 8
MAX_ROWS = 8000


@dataclass(frozen=True)
class Config:
    name: str
    dim: int
    dtype: str
    metric: str
    split: object = None        # VROD_F32_SPLIT of an f32 handle: "0", "1" or None
    id_offset: int = 0
    small: bool = False         # a plan of at most 2 000 rows (the CPU check of the model against numpy)


@dataclass
class Op:
    kind: str                   # a mutation, "reject", or a search form
    a: dict = field(default_factory=dict)

    def __repr__(self):
        def short(v):
            return f"<{v.dtype} {v.shape}>" if isinstance(v, np.ndarray) else repr(v)
        return f"Op({self.kind}, " + ", ".join(f"{k}={short(v)}" for k, v in self.a.items()) + ")"


# The committed plans: (seed, config).  The seeds were chosen on a CPU so that the conditions of test_sequence_plans.py
# hold; a change of the generator that loses one of them fails that test.
COMMITTED = (
    (11, Config("bf16-cosine-64", 64, "bf16", "cosine")),
    (12, Config("bf16-l2-72-offset", 72, "bf16", "l2", id_offset=10 ** 9)),
    (13, Config("bf16-ip-100", 100, "bf16", "ip")),
    (14, Config("f32-cosine-72-split1", 72, "f32", "cosine", split="1")),
    (15, Config("f32-l2-100-default", 100, "f32", "l2", split=None)),
    (16, Config("f32-ip-64-split0-offset", 64, "f32", "ip", split="0", id_offset=2 ** 40 + 5)),
    (17, Config("f32-l2-72-split1", 72, "f32", "l2", split="1")),
    (18, Config("f32-cosine-64-default", 64, "f32", "cosine", split=None)),
)
# Three plans of at most 2 000 rows for the CPU check of the model against numpy (test_sequence_plans.py); not run on a
# GPU.  The third is at an odd width: test_gpu_widths.py compares handles of odd and very long rows with the model.
MODEL_CHECK = (
    (18, Config("bf16-cosine-100-small", 100, "bf16", "cosine", small=True)),
    (19, Config("f32-ip-64-default-small", 64, "f32", "ip", split=None, small=True)),
    (20, Config("bf16-l2-33-small", 33, "bf16", "l2", small=True)),
)


# ------------------------------------------------------------------ search_plan.h, restated for coverage()
def graph_route(path, nq):
    """The route a search must have to be captured and replayed (search_plan.h graph_route)."""
    return path == PATH_STREAM or (path == PATH_AUTO and nq <= 4)


def builds_planes(cfg, path, filtered, N, m, nq):
    """Whether a search splits the rows of an f32 handle into planes: a split MFMA batch (search_plan.h route: AUTO sends
    an f32 batch of more than 12 queries there while the split pass is enabled), not gathered."""
    if cfg.dtype != "f32" or cfg.split == "0" or m == 0:
        return False
    if filtered and filter_route(path, cfg.dtype, N, m, nq, cfg.dim):
        return False
    return path == PATH_MFMA or (path == PATH_AUTO and nq > 12)


def is_check(op):
    return op.kind in FORMS


def apply_mutation(model, op):
    """Apply a mutation op to a ModelIndex (set_path is no state of the model).  -> what the call returns."""
    a = op.a
    if op.kind == "add":
        return model.add(a["rows"])
    if op.kind == "delete":
        return model.delete(a["ids"])
    if op.kind == "update":
        return model.update(a["ids"], a["rows"])
    if op.kind == "set_filter":
        return model.set_filter(a["allow"])
    if op.kind == "set_labels":
        return model.set_labels(a["first_id"], a["labels"])
    if op.kind == "compact":
        return model.compact()
    if op.kind == "set_path":
        return None
    raise ValueError(op.kind)


def expected(model, op):
    """What the model says a check op returns."""
    a = op.a
    if op.kind == "search":
        return model.search(a["rq"], a["k"])
    if op.kind == "search_labeled":
        return model.search_labeled(a["rq"], a["k"], a["qlabels"])
    if op.kind == "search_grouped":
        return model.search_grouped(a["rq"], a["k"])
    if op.kind == "range_search":
        return model.range_search(a["rq"], a["thr"])
    if op.kind == "search_by_ids":
        return model.search_by_ids(a["ids"], a["k"], a["exclude_self"])
    if op.kind == "knn_graph":
        return model.knn_graph(a["k"], a["first_id"], a["n"])
    if op.kind == "pipelined":
        return [model.search(rq, a["k"]) for rq in a["rq"]]
    raise ValueError(op.kind)


class _Maker:
    def __init__(self, seed, cfg, model=None):
        self.seed, self.cfg = int(seed), cfg
        self.rng = np.random.default_rng(seed)
        self.m = ModelIndex(cfg.dim, cfg.dtype, cfg.metric, cfg.id_offset) if model is None else model
        self.ops = []
        self.path = PATH_AUTO
        self.occurrence = {k: 0 for k in MUTATIONS}
        self.knn_used = 0

    # ------------------------------------------------------------------ data
    def rows(self, n):
        raw = self.rng.standard_normal((n, self.cfg.dim)).astype(np.float32)
        if self.cfg.metric == "ip":     # norms spread over e^2: a row is often not its own best match
            raw *= np.exp(self.rng.uniform(-1.0, 1.0, (n, 1))).astype(np.float32)
        return raw

    def queries(self, nq):
        """Mostly fresh vectors, some near stored rows (so that scores are not all alike)."""
        rq = self.rng.standard_normal((nq, self.cfg.dim)).astype(np.float32)
        if self.m.count:
            near = self.rng.random(nq) < 0.3
            at = self.rng.integers(0, self.m.count, nq)
            rq[near] = self.m.rows[at[near]] + 0.3 * rq[near]
        return rq

    def live_ids(self, n, rows=None):
        pool = np.flatnonzero(~self.m.deleted) if rows is None else rows[~self.m.deleted[rows]]
        n = min(n, pool.size)
        return self.rng.choice(pool, n, replace=False).astype(np.uint64) + np.uint64(self.m.offset)

    # ------------------------------------------------------------------ emit
    def emit(self, kind, **a):
        op = Op(kind, a)
        self.ops.append(op)
        return op

    def mutate(self, kind, **a):
        op = self.emit(kind, **a)
        apply_mutation(self.m, op)
        if kind == "set_path":
            self.path = a["path"]
        self.occurrence[kind] += 1
        return op

    def reject(self, what, code, **a):
        self.emit("reject", what=what, code=code, after_rq=self.queries(3), **a)

    # ------------------------------------------------------------------ mutations
    def add(self, n, check=True):
        self.mutate("add", rows=self.rows(n))
        if check:
            self.free_check("add")

    def add_outgrowing(self, check=True):
        """An add that does not fit the capacity: the smallest such size, or the next one."""
        fits = [n for n in ADD_SIZES if self.m.count + n > self.m.capacity]
        self.add(int(self.rng.choice(fits[:1 if self.cfg.small else 2])), check=check)

    def delete(self, how=None, check=True, leave=None):
        m = self.m
        how = how or str(self.rng.choice(["random", "stretch", "tail"]))
        if how == "random":
            loc = self.rng.choice(m.count, max(1, m.count // 20), replace=False)
        elif how == "stretch":
            n = int(self.rng.integers(m.count // 10, m.count // 4))
            if leave is not None:                      # a stretch long enough to leave at most `leave` live rows
                n = max(n, m.live_count() - leave + int(m.deleted.sum()))
            lo = int(self.rng.integers(0, m.count - n))
            loc = np.arange(lo, lo + n)
        else:
            loc = np.arange(m.count - int(self.rng.integers(1, max(2, m.count // 8))), m.count)
        self.mutate("delete", ids=loc.astype(np.uint64) + np.uint64(m.offset), how=how)
        if check:
            self.free_check("delete")

    def update(self, old_count):
        """Rows on both sides of old_count (rows from there on were added since the last batched search), one id twice."""
        m = self.m
        ids = np.concatenate([self.live_ids(20, np.arange(old_count)), self.live_ids(12, np.arange(old_count, m.count))])
        ids = np.concatenate([ids, ids[[0, ids.size - 1]]])
        self.rng.shuffle(ids)
        self.mutate("update", ids=ids, rows=self.rows(ids.size))

    def set_filter(self, how, check=True):
        m = self.m
        if how == "broad":
            allow = self.rng.random(m.count) < 0.5
        elif how == "narrow":
            allow = self.rng.random(m.count) < 0.01
        elif how == "short":
            allow = self.rng.random(m.count - int(self.rng.integers(1, m.count // 3))) < 0.5
        else:
            allow = None
        self.mutate("set_filter", allow=allow, how=how)
        if check:
            self.free_check("set_filter")

    def labelling(self):
        """A label on more than half of the rows, N_SMALL labels of about SMALL_ROWS rows, label 0 on the rest; nobody
        carries L_NOBODY."""
        n = self.m.count
        lab = np.zeros(n, np.uint32)
        perm = self.rng.permutation(n)
        big = n // 2 + 1 + int(self.rng.integers(0, max(1, n // 50)))
        lab[perm[:big]] = L_BIG
        at = big
        n_small = min(N_SMALL, (n - big) // (SMALL_ROWS + 1))      # (all of them from 1 800 rows on)
        for j in range(n_small):
            size = int(self.rng.integers(SMALL_ROWS - 4, SMALL_ROWS + 1))
            lab[perm[at:at + size]] = L_SMALL0 + j
            at += size
        assert at < n
        return lab

    def set_labels(self, check=True):
        self.mutate("set_labels", first_id=self.m.offset, labels=self.labelling())
        if check:
            self.free_check("set_labels")

    def set_path(self, path, check=False):
        self.mutate("set_path", path=int(path))
        if check:
            self.free_check("set_path")

    # ------------------------------------------------------------------ checks
    def shape(self, nq=None):
        nq = int(self.rng.choice(NQS)) if nq is None else nq
        return nq, int(self.rng.choice(KS))

    def query_labels(self, nq):
        present = np.unique(self.m.labels)
        pool = np.concatenate([[L_BIG, L_NOBODY, 0], present[(present >= L_SMALL0) & (present < L_SMALL0 + N_SMALL)]])
        q = self.rng.choice(pool, nq).astype(np.uint32)
        q[0] = L_BIG                                   # the dense stage
        if nq > 1:
            q[1] = L_NOBODY
        if nq > 2:
            q[2] = pool[-1]                            # the narrow stage
        return q

    def check(self, form, nq=None, k=None):
        m = self.m
        nq0, k0 = self.shape(nq)
        k = k0 if k is None else k
        if form == "search":
            return self.emit("search", rq=self.queries(nq0), k=k)
        if form == "search_labeled":
            nq0 = max(nq0, 3)
            return self.emit("search_labeled", rq=self.queries(nq0), k=k, qlabels=self.query_labels(nq0))
        if form == "search_grouped":
            return self.emit("search_grouped", rq=self.queries(min(nq0, 40)), k=k)
        if form == "range_search":
            rq = self.queries(min(nq0, 40))
            return self.emit("range_search", rq=rq, thr=self.thresholds(rq))
        if form == "search_by_ids":
            ids = self.live_ids(nq0)
            if ids.size > 2:
                ids[1] = ids[0]                        # an id may repeat
            return self.emit("search_by_ids", ids=ids, k=k, exclude_self=bool(self.rng.integers(2)))
        if form == "knn_graph":
            self.knn_used += 1
            if m.count <= KNN_MAX_ROWS:
                return self.emit("knn_graph", k=min(k, 10), first_id=None, n=None)
            n = 300                                    # a handle too large for the whole graph here: a stretch of it
            return self.emit("knn_graph", k=min(k, 10), first_id=m.offset + int(self.rng.integers(0, m.count - n)), n=n)
        if form == "pipelined":
            return self.emit("pipelined", rq=np.stack([self.queries(PIPE_NQ) for _ in range(PIPE_CHAIN)]), k=PIPE_K)
        raise ValueError(form)

    def thresholds(self, rq):
        """From the model's own ranking: query q gets the score of a random rank, so that it returns between no row and a
        few hundred."""
        m = self.m
        elig = m.filter_count()
        thr = np.zeros(rq.shape[0], np.float32)
        if elig == 0:
            return thr
        kk = min(elig, 300)
        _, sc = m.search(rq, kk)
        for q in range(rq.shape[0]):
            t = int(self.rng.integers(0, kk + 1))
            if t:
                thr[q] = sc[q, t - 1]
            else:                                      # better than the best row: nothing qualifies
                best = sc[q, 0]
                thr[q] = best - abs(best) - 1 if m.form == 1 else best + abs(best) + 1
        return thr

    def free_check(self, kind):
        """The check behind a mutation of `kind`: its form rotates with the seed and the mutation's occurrence."""
        at = self.seed + 3 * MUTATIONS.index(kind) + self.occurrence[kind] - 1
        for step in range(len(FORMS)):
            form = FORMS[(at + step) % len(FORMS)]
            if form == "knn_graph" and (self.m.count > KNN_MAX_ROWS or self.knn_used >= KNN_PER_PLAN):
                continue
            return self.check(form)

    # ------------------------------------------------------------------ rejected ops
    def reject_values(self):
        m = self.m
        what = str(self.rng.choice(["add_nan", "update_nan", "update_deleted"]))
        if what == "add_nan":
            rows = self.rows(int(self.rng.choice([1, 37])))
            rows[-1, self.cfg.dim // 2] = np.nan
            self.reject(what, 2, rows=rows)
            try:
                m.add(rows)                            # (index_add grows the capacity before it looks at the values)
            except ModelError:
                pass
        elif what == "update_nan":
            ids = self.live_ids(5)
            rows = self.rows(ids.size)
            rows[2, 0] = np.inf
            self.reject(what, 2, ids=ids, rows=rows)
        else:
            ids = self.live_ids(5)
            ids[3] = np.flatnonzero(m.deleted)[0] + m.offset
            self.reject(what, 1, ids=ids, rows=self.rows(ids.size))

    def reject_ids(self):
        m = self.m
        if self.rng.integers(2) and m.deleted.any():
            ids = self.live_ids(4)
            ids[2] = np.flatnonzero(m.deleted)[-1] + m.offset
            self.reject("byid_deleted", 1, ids=ids, k=10, exclude_self=bool(self.rng.integers(2)))
        else:
            self.reject("compact_map_len", 1, map_len=m.count + int(self.rng.choice([-1, 1])))

    def reject_pending(self):
        m = self.m
        which = str(self.rng.choice(["add", "delete", "update", "set_filter", "set_labels", "compact"]))
        ids = self.live_ids(3)
        inner = {"add": dict(rows=self.rows(2)), "delete": dict(ids=ids), "update": dict(ids=ids, rows=self.rows(ids.size)),
                 "set_filter": dict(allow=np.ones(m.count, bool)), "set_labels": dict(first_id=m.offset, labels=np.full(5, 9, np.uint32)),
                 "compact": dict()}[which]
        self.reject("pending_" + which, 1, rq=self.queries(PIPE_NQ), op=Op(which, inner))

    # ------------------------------------------------------------------ the plan
    def make(self):
        rng, m, small = self.rng, self.m, self.cfg.small
        # A
        self.add(1500 if not small else 300, check=False)
        self.add(300 if not small else 37)
        for kind in rng.permutation(["set_labels", "delete", "set_filter"]):
            if kind == "set_labels":
                self.set_labels()
            elif kind == "delete":
                self.delete("random")
            else:
                self.set_filter(str(rng.choice(["broad", "short"])))
        # B
        for block in rng.permutation(["gather", "update", "reject"]):
            if block == "gather":
                self.set_path(PATH_GATHER)
                self.check("search", nq=int(rng.choice([3, 40])))
                self.check("search_labeled")
                self.check("search", nq=int(rng.choice([3, 40])))
                self.set_path(int(rng.choice([PATH_AUTO, PATH_MFMA])), check=True)
            elif block == "update":
                assert self.path in (PATH_AUTO, PATH_MFMA)     # (the routes that build the planes)
                self.check("search", nq=int(rng.choice([40, 300])))
                old = m.count
                self.add(int(rng.choice([37, 300])) if m.count + 300 <= m.capacity and not small else 37, check=False)
                self.update(old)
                self.check("search", nq=int(rng.choice([40, 300])))
                self.free_check("update")
            else:
                self.reject_values()
        self.add_outgrowing(check=False)               # (the rejected op behind it is followed by a search of its own)
        self.reject_ids()
        self.add_outgrowing()
        # H
        if self.path != PATH_STREAM:
            self.set_path(PATH_STREAM)
        self.check("pipelined")
        for i in range(2):
            self.check(FORMS[1 + (self.seed + 2 * i) % 4], nq=int(rng.choice([3, 9])))
            self.check("pipelined")
        # C
        clear = bool(rng.integers(2))
        if not clear:
            self.set_path(int(rng.choice([PATH_AUTO, PATH_MFMA, PATH_EXACT, PATH_GATHER])))
        how = "stretch" if rng.integers(2) else "tail"
        if FORMS[(self.seed + 3 * MUTATIONS.index("compact")) % len(FORMS)] == "knn_graph" and self.knn_used < KNN_PER_PLAN:
            self.delete("stretch", check=False, leave=KNN_MAX_ROWS - 200)     # the graph is the check behind this compaction
        else:
            self.delete(how, check=False)
        self.mutate("compact")
        self.free_check("compact")
        self.add(int(rng.choice(ADD_SIZES[:3])))
        self.reject_pending()
        if clear:
            self.set_filter("none")
        self.set_filter("narrow", check=False)         # few eligible rows: a k above them
        self.check(FORMS[int(rng.choice([0, 1, 2, 4]))], k=m.filter_count() + 7)
        assert m.count <= MAX_ROWS
        return self.ops


def make_plan(seed, config):
    return _Maker(seed, config).make()


def every_form(seed, config, model, nqs=(3, 40), k=10):
    """One check op of every search form for the model's present state (the end of a plan, the scripted orderings):
    the query forms at each of `nqs`, by ids with and without the row itself, the graph (a stretch of it on a large handle)
    and the pipelined chain."""
    mk = _Maker(seed, config, model)
    for nq in nqs:
        mk.check("search", nq=nq, k=k)
        mk.check("search_labeled", nq=nq, k=k)
        mk.check("search_grouped", nq=nq, k=k)
        mk.check("range_search", nq=nq)
    if model.live_count():
        for ex in (False, True):
            mk.check("search_by_ids", nq=nqs[-1], k=k).a["exclude_self"] = ex
    if model.count:
        mk.check("knn_graph", k=k)
    mk.check("pipelined")
    return mk.ops


def coverage(plan, config):
    """Replay a plan on the model alone and count the orderings it reaches (the issue's counters (a) .. (h))."""
    m = ModelIndex(config.dim, config.dtype, config.metric, config.id_offset)
    cov = {"a": 0, "b": 0, "c": 0, "d": 0, "e": {}, "f": 0, "g": 0, "h": {f: 0 for f in FORMS[1:5]}, "k_above": 0,
           "steps": len(plan), "max_rows": 0, "knn": 0, "labellings": 0}
    labelled = compacted = batched = False
    covered = 0
    path = PATH_AUTO
    last_mut = None
    g_state = 0
    piped_since_mut = False
    prev = None
    for op in plan:
        if op.kind == "reject":
            cov["f"] += 1
            w = op.a["what"]
            try:
                if w == "add_nan":
                    m.add(op.a["rows"])
                elif w in ("update_nan", "update_deleted"):
                    m.update(op.a["ids"], op.a["rows"])
                elif w == "byid_deleted":
                    m.search_by_ids(op.a["ids"], op.a["k"], op.a["exclude_self"])
                elif w == "compact_map_len":
                    m.compact(op.a["map_len"])
                else:
                    raise ModelError(1, "pending")
                raise AssertionError(f"the model accepts {op}")
            except ModelError as e:
                assert e.code == op.a["code"], op
        elif is_check(op):
            key = (op.kind, last_mut)
            cov["e"][key] = cov["e"].get(key, 0) + 1
            nq = op.a["rq"].shape[0] if op.kind == "search" else 0
            N, elig = m.count, m.filter_count()
            gather = op.kind == "search" and filter_route(path, config.dtype, N, elig, nq, config.dim) and (path == PATH_GATHER or m.allow is not None)
            if gather and g_state == 2:
                cov["g"] += 1
            g_state = 1 if gather else 2 if (op.kind == "search_labeled" and g_state >= 1) else g_state
            if nq > 32 and builds_planes(config, path, m.allow is not None, N, elig, nq):
                batched, covered = True, m.count
            if op.kind == "pipelined":
                # a chain is captured and replayed only on a graph route, not gathered, with a row to return
                graphable = (graph_route(path, PIPE_NQ) and elig > 0 and path != PATH_GATHER
                             and not (m.allow is not None and filter_route(path, config.dtype, N, elig, PIPE_NQ, config.dim)))
                if graphable and piped_since_mut and prev in cov["h"]:
                    cov["h"][prev] += 1
                piped_since_mut = graphable
            if op.kind == "knn_graph":
                cov["knn"] += 1
                assert m.count <= KNN_MAX_ROWS
            if "k" in op.a and op.kind != "pipelined" and op.a["k"] > m.filter_count():
                cov["k_above"] += 1
        else:
            if op.kind == "add":
                state = m.deleted.any() and m.allow is not None and labelled
                if m.add(op.a["rows"]):
                    cov["a"] += bool(state)
                    batched, covered = False, 0        # (the growth frees the planes)
                cov["c"] += compacted
            elif op.kind == "update":
                loc = (np.asarray(op.a["ids"], np.uint64) - np.uint64(m.offset)).astype(np.int64)
                cov["d"] += bool(config.dtype == "f32" and batched and (loc >= covered).any() and (loc < covered).any())
                apply_mutation(m, op)
            elif op.kind == "compact":
                cov["b"] += bool(m.allow is not None and labelled)
                apply_mutation(m, op)
                compacted, covered = True, 0           # (planes_rows = 0: the planes cover no row)
            else:
                apply_mutation(m, op)
            if op.kind == "set_labels":
                labelled = True
                lab, n = m.labels, m.count
                sizes = np.array([(lab == L_SMALL0 + j).sum() for j in range(N_SMALL)])
                cov["labellings"] += bool((lab == L_BIG).sum() > n // 2 and (sizes >= SMALL_ROWS - 4).all() and (lab == 0).any()
                                          and not (lab == L_NOBODY).any())
            piped_since_mut = False                    # (a graph's key holds the path, the corpus, its size and the mask)
            if op.kind == "set_path":
                path = op.a["path"]
            else:
                g_state = 0
            last_mut = op.kind
        cov["max_rows"] = max(cov["max_rows"], m.count)
        prev = op.kind
    cov["final_rows"] = m.count
    return cov
