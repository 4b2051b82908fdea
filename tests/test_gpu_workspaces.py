"""GPU tests of the workspaces the derived searches share (DESIGN.md "Shared workspaces").

The labelled, tagged, grouped, multi-vector, diversified, by-id, combined and candidate-list searches and the k-NN graph
keep one buffer per role on the handle -- the host forms' staged queries and arguments, the first-stage lists, the
result columns -- so a buffer grown by one call is reused, larger and smaller, by the next.  Every result is exact,
hence the check: a long-lived handle that runs all of them in several orders and sizes must return, bit for bit, what a
fresh handle built from the same data returns for the same call; a fresh handle has never shared anything.

One corpus of 6 000 rows, d = 64, per dtype: a label on 2 500 rows (a batch of many queries scans it densely), one on 600,
a heavy label whose 500 rows are perturbations of query 0 (that query's first list holds one label: the grouped search's
dense stage finishes it), 100 labels of about 20 rows and label 0 on the rest; tags of six bits with falling
probability; 150 deleted rows and a filter that allows nine rows of ten.
"""
import numpy as np
import pytest

from support import DT, va, O, takes_segments, oracle_over, eligible_rows, assert_same, same_f32, PATH_AUTO  # noqa: F401

pytestmark = pytest.mark.gpu

N, DIM = 6_000, 64
L_HALF, L_TENTH, L_HEAVY, SMALL0, N_SMALL = 4_000_000_000, 1000, 77, 10_000, 100
BIG, SMALL = (192, 100), (3, 5)                    # (nq, k) of a call


class World:
    def __init__(self, dtype, metric):
        rng = np.random.default_rng(20262 + DT[dtype])
        self.dtype, self.metric = dtype, metric
        self.raw = rng.standard_normal((N, DIM)).astype(np.float32)
        self.rq = rng.standard_normal((BIG[0], DIM)).astype(np.float32)
        perm = rng.permutation(N)
        self.labels = np.zeros(N, np.uint32)
        at = 0
        for value, n in [(L_HALF, 2_500), (L_TENTH, 600), (L_HEAVY, 500)] + [(SMALL0 + j, int(rng.integers(12, 29))) for j in range(N_SMALL)]:
            self.labels[perm[at:at + n]] = value
            at += n
        assert at < N
        heavy = np.flatnonzero(self.labels == L_HEAVY)
        self.raw[heavy] = self.rq[0] + 0.05 * rng.standard_normal((heavy.size, DIM)).astype(np.float32)
        self.tags = np.zeros(N, np.uint64)
        for b, p in enumerate((0.5, 0.3, 0.3, 0.3, 0.05, 0.01)):
            self.tags |= (rng.random(N) < p).astype(np.uint64) << np.uint64(b)
        self.deleted = rng.choice(N, 150, replace=False)
        self.allow = rng.random(N) < 0.9
        self.live = np.setdiff1d(np.arange(N), self.deleted)
        self.rng_seed = 7 + DT[dtype]

    def make(self, va):
        ix = va.Index(DIM, self.dtype, self.metric)
        ix.add(self.raw)
        ix.set_labels(0, self.labels)
        ix.set_tags(0, self.tags)
        ix.delete(self.deleted)
        ix.set_filter(self.allow)
        return ix

    # ---- the arguments of a call of `size`, the same whichever handle it goes to
    def qlabels(self, nq):
        q = [L_HALF] * (nq * 2 // 3) + [L_TENTH, SMALL0 + 3, 5]          # (5: no row carries it)
        q += [SMALL0 + j % N_SMALL for j in range(nq)]
        return np.array(q[:nq], np.uint32)

    def preds(self, nq):
        p = np.zeros((nq, 3), np.uint64)
        p[:, 0] = 1                                                      # any of bit 0: half of the rows
        p[nq // 2:] = (0, 0b1110, 0)                                     # all of bits 1..3: about 3 rows in 100
        p[-1] = (0, 1, 1)                                                # unsatisfiable
        return p

    def lens(self, nq):
        return [(1, 2, 31, 32, 33, 5)[q % 6] for q in range(max(1, nq // 8))]

    def ids_of(self, nq, seed):
        return np.random.default_rng(self.rng_seed + seed).choice(self.live, nq, replace=False).astype(np.uint64)

    def combined(self, nq):
        terms = self.ids_of(2 * nq, 1)
        excl = np.concatenate([self.ids_of(2 * nq, 2), terms[::2]])      # three excluded ids per query, one of them a term
        w = np.linspace(-1.0, 1.5, 2 * nq).astype(np.float32)
        vw = np.linspace(0.5, 2.0, nq).astype(np.float32)
        return terms, w, np.arange(nq + 1, dtype=np.uint32) * 2, vw, excl.reshape(3, nq).T.copy().reshape(-1), np.arange(nq + 1, dtype=np.uint32) * 3

    def candidates(self, nq):
        rng = np.random.default_rng(self.rng_seed + 3)
        lens = rng.integers(0, 2 * BIG[1] if nq > 8 else 10, nq)
        lims = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        return rng.integers(0, N + 50, int(lims[-1])).astype(np.uint64), lims   # (repeats, deleted rows and ids past the rows included)


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host(*tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in tensors)


def calls(va, W):
    """name -> f(ix, (nq, k)): every host form and every device form of the derived searches, and the graph."""
    def q(nq):
        return W.rq[:nq]

    def mv(nq):
        lens = W.lens(nq)
        return np.resize(W.rq, (sum(lens), DIM)), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)

    def comb_dev(ix, nq, k):
        t, w, tl, vw, x, xl = W.combined(nq)
        return host(*ix.search_combined_device(k, dev(tl), dev(t), dev(w), dev(q(nq)), dev(vw), dev(xl), dev(x), exclude_terms=True))

    def comb(ix, nq, k):
        t, w, tl, vw, x, xl = W.combined(nq)
        return ix.search_combined(k, t, w, tl, q(nq), vw, x, xl, exclude_terms=True)

    def graph(ix, nq, k):
        batch = va.index.KNN_BATCH[DT[W.dtype]]
        return ix.knn_graph(min(k, 10), 0, 2 * batch + 300 if nq > 8 else 300)   # three batches: both sets of lists, a partial tail

    return {
        "labeled": lambda ix, nq, k: ix.search_labeled(q(nq), k, W.qlabels(nq)),
        "labeled_device": lambda ix, nq, k: host(*ix.search_labeled_device(dev(q(nq)), k, dev(W.qlabels(nq)))),
        "tagged": lambda ix, nq, k: ix.search_tagged(q(nq), k, W.preds(nq)),
        "tagged_device": lambda ix, nq, k: host(*ix.search_tagged_device(dev(q(nq)), k, dev(W.preds(nq)))),
        "grouped": lambda ix, nq, k: ix.search_grouped(q(nq), k),
        "grouped_device": lambda ix, nq, k: host(*ix.search_grouped_device(dev(q(nq)), k)),
        "grouped_device_no_labels": lambda ix, nq, k: host(*ix.search_grouped_device(dev(q(nq)), k, want_labels=False)),
        "multivec": lambda ix, nq, k: ix.search_multivec(mv(nq)[0], k // 2 + 1, mv(nq)[1]),
        "multivec_device": lambda ix, nq, k: host(*ix.search_multivec_device(dev(mv(nq)[0]), dev(mv(nq)[1]), k // 2 + 1)),
        "multivec_device_no_found": lambda ix, nq, k: host(*ix.search_multivec_device(dev(mv(nq)[0]), dev(mv(nq)[1]), k // 2 + 1, want_found=False)),
        "diverse": lambda ix, nq, k: ix.search_diverse(q(nq), k, 2 * k, 0.5),
        "diverse_device": lambda ix, nq, k: host(*ix.search_diverse_device(dev(q(nq)), k, 2 * k, 0.5)),
        "diverse_device_no_mmr": lambda ix, nq, k: host(*ix.search_diverse_device(dev(q(nq)), k, 2 * k, 0.5, want_mmr=False)),
        "by_ids": lambda ix, nq, k: ix.search_by_ids(W.ids_of(nq, 0), k, exclude_self=True),
        "by_ids_device": lambda ix, nq, k: host(*ix.search_by_ids_device(dev(W.ids_of(nq, 0)), k, exclude_self=True)),
        "combined": lambda ix, nq, k: comb(ix, nq, k),
        "combined_device": lambda ix, nq, k: comb_dev(ix, nq, k),
        "candidates": lambda ix, nq, k: ix.search_candidates(q(nq), k, *W.candidates(nq)),
        "candidates_device": lambda ix, nq, k: host(*ix.search_candidates_device(dev(q(nq)), k, dev(W.candidates(nq)[1]), dev(W.candidates(nq)[0]))),
        "score_candidates": lambda ix, nq, k: (ix.score_candidates(q(nq), *W.candidates(nq)),),
        "score_candidates_device": lambda ix, nq, k: host(ix.score_candidates_device(dev(q(nq)), dev(W.candidates(nq)[1]), dev(W.candidates(nq)[0]))),
        "knn_graph": graph,
    }


def same_result(got, want, what):
    assert len(got) == len(want), what
    for j, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, f"{what}: column {j}"
        elif np.asarray(a).dtype == np.float32:
            assert same_f32(a, b), f"{what}: column {j} differs"
        else:
            assert np.array_equal(a, b), f"{what}: column {j} differs"


@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "l2")])
def test_shared_buffers_across_calls(va, dtype, metric):
    W = World(dtype, metric)
    C = calls(va, W)
    # the routes the big calls take, from the library's own rules and reports
    ql = W.qlabels(BIG[0])
    ok = np.zeros(N, bool)
    ok[eligible_rows(N, W.allow, W.deleted)] = True
    seg = {int(L): takes_segments(PATH_AUTO, dtype, N, int(((W.labels == L) & ok).sum()), int((ql == L).sum()), DIM) for L in np.unique(ql)}
    assert not seg[L_HALF] and seg[SMALL0 + 3], seg            # a labelled batch holds a dense group and segmented ones
    want = {}
    for size in (BIG, SMALL):
        for name, f in C.items():
            with W.make(va) as fresh:
                want[name, size] = f(fresh, *size)
                if name == "grouped":
                    fb = fresh.last_stats()["fallback_queries"]
                    assert (0 < fb) if size == BIG else (fb < size[0]), (size, fb)   # the dense stage ran / did not run for all
                if name == "multivec":
                    assert fresh.last_multivec()["k1"] > 0     # the candidate route's first-stage lists were written
    order = [(n, s) for s in (BIG, SMALL) for n in C]
    with W.make(va) as ix:
        for name, size in order + order[::-1]:
            same_result(C[name](ix, *size), want[name, size], f"{name} {size} on the long-lived handle")


def test_create_and_destroy(va, O):
    """Every workspace grown, then the handle destroyed, several times over, a composite handle among them: a crash and
    double-free check, not a memory measurement."""
    for it in range(4):
        W = World(("f32", "bf16")[it % 2], ("cosine", "l2")[it % 2])
        C = calls(va, W)
        ix = W.make(va)
        for name, f in C.items():
            f(ix, 8, 6)                                        # (a failed call raises)
        with va.Index(DIM, "bf16", "cosine", devices=[0, 0]) as mx:
            mx.add(W.raw)
            mx.search(W.rq[:3], 5)
            mx.range_search(W.rq[:2], 0.5)
        if it < 3:
            ix.close()
    ids, sc = ix.search(W.rq[:9], 10)
    oi, osc = oracle_over(O, W.raw, W.rq[:9], 10, W.dtype, W.metric, eligible_rows(N, W.allow, W.deleted))
    ix.close()
    assert_same(ids, sc, oi, osc, "the last handle")
