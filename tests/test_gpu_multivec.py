"""GPU tests of the multi-vector search (vrod_search_multivec) against the model in tests/multivec_model.py.

The contract: S(q, L) = the fp32 sum, in vector order from +0.0, of the best canonical score of each of the query's
vectors over the eligible rows of label L; the k best labels per query, a NaN S last, ties by the smaller label; slots
past the labels with an eligible row are (0, NaN); found = the filled slots.  Labels and found must be equal, score bits
equal (a NaN matches any NaN).

Parity corpus: 7 000 rows; the labels are scattered, non-contiguous values, 0 and 0xFFFFFFFF among them; documents of 1
to 40 rows, several of exactly one row, and one broad label on about 2 000 rows.  Every dtype x metric, every dim of
{1, 3, 64, 100, 768}, every query length of {1, 2, 31, 32, 33, 256}, nq of {1, 3, 17} with mixed lengths, k of {1, 10,
more than the labels}, on the default path, under VROD_PATH_EXACT (the dense route alone) and with STREAM and MFMA forced;
the model's S table is computed once per case and shared by every path and k.

Routes (vrod_index_last_multivec): a topical corpus on which the model says every query is certifiable, an unstructured
one on which none is, and a mixed batch; the model applies multivec_plan.h's rules (no retry exists) to the oracle's own
top-k1 lists, and the premise is asserted before the library is asked.
"""
import numpy as np
import pytest

from multivec_model import MultivecModel, first_k
from support import PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, va, assert_scores_same  # noqa: F401

pytestmark = pytest.mark.gpu

PATHS = {"auto": PATH_AUTO, "exact": PATH_EXACT, "stream": PATH_STREAM, "mfma": PATH_MFMA}
N = 7_000
L_BROAD, N_BROAD = 0xFFFFFFFF, 2_000
LENS17 = [1, 2, 31, 32, 33, 256, 1, 2, 5, 8, 3, 33, 32, 31, 2, 1, 7]
# (dtype, metric, dim, query lengths): every dtype x metric, every dim, nq of 1, 3 and 17
CASES = {
    "f32-cosine-64": ("f32", "cosine", 64, LENS17),
    "f32-l2-100": ("f32", "l2", 100, LENS17),
    "f32-ip-3": ("f32", "ip", 3, LENS17),
    "bf16-cosine-768": ("bf16", "cosine", 768, [33, 2, 256]),
    "bf16-l2-1": ("bf16", "l2", 1, LENS17),
    "bf16-ip-64": ("bf16", "ip", 64, [31, 1, 32]),
    "f32-cosine-768": ("f32", "cosine", 768, [33]),
    "bf16-cosine-100": ("bf16", "cosine", 100, [256]),
}
K_ABOVE = 1_000   # more than the corpus has labels


def assert_same(got, want, what=""):
    (lab, sc, found), (ol, osc, of) = got, want
    assert np.array_equal(found, of), f"{what}: found differs at {np.argwhere(found != of)[:5]}"
    assert np.array_equal(lab, ol), f"{what}: labels differ at {np.argwhere(lab != ol)[:5]}"
    assert_scores_same(sc, osc, what)


def parity_labels(rng, n=N):
    """Scattered label values; documents of 1 .. 40 rows, ten of one row, one broad label, label 0 present."""
    values = np.unique(np.concatenate([[0], rng.integers(1, 0xFFFFFFFE, 2_000, dtype=np.uint64)])).astype(np.uint32)
    rng.shuffle(values[1:])
    lab = np.full(n, L_BROAD, np.uint32)
    at, v = N_BROAD, 0
    while at < n:
        size = 1 if v < 10 else int(rng.integers(1, 41))
        lab[at:at + size] = values[v]
        at, v = at + size, v + 1
    return lab[rng.permutation(n)]       # documents are not contiguous runs of rows


def lims_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


def make_index(va, model, raw, labels=None):
    ix = va.Index(model.dim, model.dtype, model.metric)
    ix.add(raw)
    model.add(raw)
    if labels is not None:
        ix.set_labels(0, labels)
        model.set_labels(0, labels)
    return ix


def device_form(ix, vec, lims, k):
    import torch
    dv = torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32)).cuda()
    dl = torch.from_numpy(np.asarray(lims, dtype=np.uint32).view(np.int32)).cuda()
    lab, sc, found = ix.search_multivec_device(dv, dl, k)
    torch.cuda.synchronize()
    return lab.cpu().numpy().view(np.uint32), sc.cpu().numpy(), found.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def parity(va):
    """Per case, built on first use and kept: the handle, the model, the query set and the model's S table."""
    cache = {}

    def get(name):
        if name not in cache:
            dtype, metric, dim, lens = CASES[name]
            rng = np.random.default_rng(sum(map(ord, name)))
            raw = rng.standard_normal((N, dim)).astype(np.float32)
            vec = rng.standard_normal((int(np.sum(lens)), dim)).astype(np.float32)
            model = MultivecModel(dim, dtype, metric)
            ix = make_index(va, model, raw, parity_labels(rng))
            lims = lims_of(lens)
            present, S = model.scores_multivec(vec, lims)
            assert present.size < K_ABOVE and 0 in present and L_BROAD in present
            cache[name] = (ix, model, vec, lims, present, S)
        return cache[name]
    yield get
    for ix, *_ in cache.values():
        ix.close()


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_model(parity, case, path):
    ix, model, vec, lims, present, S = parity(case)
    ix.set_path(PATHS[path])
    try:
        for k in (1, 10, K_ABOVE):
            want = model.rank(present, S, k)
            got = ix.search_multivec(vec, k, lims=lims)
            assert_same(got, want, f"{case} {path} k={k} host form")
            mv, st = ix.last_multivec(), ix.last_stats()
            assert mv["nq"] == lims.size - 1 and mv["vectors"] == lims[-1] and st["nq"] == lims.size - 1 and st["k"] == k
            assert mv["certified_queries"] + mv["dense_queries"] == mv["nq"]
            if path == "exact":
                assert mv["dense_queries"] == mv["nq"] and mv["k1"] == 0 and st["path"] == PATH_EXACT
            else:
                assert mv["k1"] == first_k(k, N)
            assert st["fallback_queries"] >= mv["dense_queries"]
            if k == 10:
                assert_same(device_form(ix, vec, lims, k), got, f"{case} {path} k={k} device form")
        got = ix.search_multivec([vec[lims[q]:lims[q + 1]] for q in range(lims.size - 1)], 10)   # the list form
        assert_same(got, model.rank(present, S, 10), f"{case} {path} list form")
    finally:
        ix.set_path(PATH_AUTO)


# ---------------------------------------------------------------------------------------------------------------- state
@pytest.fixture()
def small(va):
    """A fresh 3 000-row handle (f32 cosine, d = 64) with 150 documents, its model and two queries."""
    rng = np.random.default_rng(77)
    raw = rng.standard_normal((3_000, 64)).astype(np.float32)
    labels = (rng.integers(0, 150, 3_000).astype(np.uint32) * np.uint32(7_919)) ^ np.uint32(0x5A5A0000)
    model = MultivecModel(64, "f32", "cosine")
    ix = make_index(va, model, raw, labels)
    vec = raw[rng.integers(0, 3_000, 9)] + 0.3 * rng.standard_normal((9, 64)).astype(np.float32)
    yield ix, model, vec.astype(np.float32), lims_of([4, 5]), rng
    ix.close()


def check_both_routes(ix, model, vec, lims, what, ks=(1, 5, 200)):
    for path in (PATH_AUTO, PATH_EXACT):
        ix.set_path(path)
        for k in ks:
            assert_same(ix.search_multivec(vec, k, lims=lims), model.search_multivec(vec, lims, k), f"{what} path={path} k={k}")
    ix.set_path(PATH_AUTO)


def test_after_deletes_filter_update_compact(small):
    ix, model, vec, lims, rng = small
    lab, _, _ = model.search_multivec(vec, lims, 2)
    whole, part = lab[0, 0], lab[0, 1]                      # the best document loses every row, the second one some
    gone = np.concatenate([np.flatnonzero(model.labels == whole), np.flatnonzero(model.labels == part)[::2]]).astype(np.uint64)
    ix.delete(gone); model.delete(gone)
    check_both_routes(ix, model, vec, lims, "after deletes")
    lab, _, found = ix.search_multivec(vec, 200, lims=lims)
    assert whole not in lab[0, :found[0]] and part in lab[0, :found[0]]
    # a filter that hides the best rows of the now best document: its M comes from the rows that are left
    best = model.search_multivec(vec, lims, 1)[0][0, 0]
    rows = np.flatnonzero((model.labels == best) & ~model.deleted)
    pv = model._queries(vec[:4])
    top = model._topk(rows, pv, 1)[0][:, 0].astype(np.int64)
    allow = np.ones(model.count, bool)
    allow[top] = False
    ix.set_filter(allow); model.set_filter(allow)
    check_both_routes(ix, model, vec, lims, "under a filter")
    ix.set_filter(None); model.set_filter(None)
    ids = np.flatnonzero(~model.deleted)[:40].astype(np.uint64)
    new = rng.standard_normal((40, 64)).astype(np.float32)
    new[:4] = vec[:4]                                       # four rows become the query's own vectors
    ix.update(ids, new); model.update(ids, new)
    check_both_routes(ix, model, vec, lims, "after update")
    ix.compact(); model.compact()
    check_both_routes(ix, model, vec, lims, "after compact")


def test_add_and_set_labels_invalidate_the_document_index(small):
    ix, model, vec, lims, rng = small
    check_both_routes(ix, model, vec, lims, "before", ks=(5,))
    more = np.concatenate([vec, rng.standard_normal((50, 64)).astype(np.float32)])   # later rows carry label 0
    ix.add(more); model.add(more)
    check_both_routes(ix, model, vec, lims, "after add")
    assert ix.search_multivec(vec, 1, lims=lims)[0][0, 0] == 0     # the query's own vectors, under label 0, win
    relabel = rng.integers(1_000_000, 1_000_040, model.count).astype(np.uint32)
    ix.set_labels(0, relabel); model.set_labels(0, relabel)
    check_both_routes(ix, model, vec, lims, "after set_labels")


def test_unlabelled_empty_and_no_eligible_row(va):
    rng = np.random.default_rng(5)
    raw = rng.standard_normal((500, 16)).astype(np.float32)
    vec, lims = rng.standard_normal((5, 16)).astype(np.float32), lims_of([2, 3])
    for dtype, metric in (("f32", "l2"), ("bf16", "ip")):
        model = MultivecModel(16, dtype, metric)
        with va.Index(16, dtype, metric) as ix:
            lab, sc, found = ix.search_multivec(vec, 3, lims=lims)          # an empty handle
            assert not lab.any() and np.isnan(sc).all() and not found.any()
            ix.add(raw); model.add(raw)
            check_both_routes(ix, model, vec, lims, "labels never set", ks=(1, 3))   # one document, label 0
            assert ix.search_multivec(vec, 3, lims=lims)[2].tolist() == [1, 1]
            ix.set_filter(np.zeros(500, bool))
            bad = np.full((2, 16), np.nan, np.float32)                      # not looked at: no eligible row
            lab, sc, found = ix.search_multivec(bad, 3, lims=[0, 1, 2])
            assert not lab.any() and np.isnan(sc).all() and not found.any()
            assert ix.last_multivec()["dense_queries"] == 0 and ix.last_multivec()["certified_queries"] == 0


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(va, small):
    import ctypes as C
    import torch
    ix, model, vec, lims, rng = small
    L = va.load()
    lab = np.full((2, 3), 0xABCDEF01, np.uint32)
    sc = np.full((2, 3), 123.5, np.float32)
    found = np.full(2, 77, np.uint32)

    def call(v, la, h=None):
        v = np.ascontiguousarray(v, dtype=np.float32)
        la = np.ascontiguousarray(la, dtype=np.uint32)
        rc = L.vrod_search_multivec(h or ix._h, v.ctypes.data_as(C.c_void_p), la.ctypes.data_as(C.c_void_p), la.size - 1, 3,
                                    lab.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p))
        assert (lab == 0xABCDEF01).all() and (sc == 123.5).all() and (found == 77).all(), "a refused call wrote to the outputs"
        return rc

    big = rng.standard_normal((258, 64)).astype(np.float32)
    assert call(vec, [1, 4, 9]) == 1                       # lims[0] != 0
    assert call(vec, [0, 5, 4]) == 1                       # decreasing
    assert call(vec, [0, 0, 9]) == 1                       # a query without a vector
    assert call(big, [0, 257, 258]) == 1                   # 257 vectors
    nanv = vec.copy()
    nanv[7, 3] = np.nan
    assert call(nanv, lims) == 2                           # NaN in the second query: nothing written, not even query 0
    nanv[7, 3] = np.inf
    assert call(nanv, lims) == 2
    for path in (PATH_EXACT, PATH_AUTO):
        ix.set_path(path)
        nanv[7, 3] = np.nan
        assert call(nanv, lims) == 2
    # while a search is pending
    dq = torch.from_numpy(vec[:2].copy()).cuda()
    oi = torch.empty((2, 4), dtype=torch.int64, device="cuda")
    os_ = torch.empty((2, 4), dtype=torch.float32, device="cuda")
    ix.search_begin_device(dq, 4, oi, os_)
    try:
        assert call(vec, lims) == 1
        dl = torch.from_numpy(lims.view(np.int32).copy()).cuda()
        with pytest.raises(va.VrodError) as e:
            ix.search_multivec_device(torch.from_numpy(vec).cuda(), dl, 3)
        assert e.value.code == 1
    finally:
        ix.search_end()
    # a multi-device handle (a repeated device id, as tests/test_gpu_multidevice.py makes them)
    with va.Index(64, "f32", "cosine", devices=[0, 0]) as mix:
        mix.add(rng.standard_normal((300, 64)).astype(np.float32))
        assert call(vec, lims, mix._h) == 6
    # and the call still works afterwards
    assert_same(ix.search_multivec(vec, 3, lims=lims), model.search_multivec(vec, lims, 3), "after the refusals")


# ---------------------------------------------------------------------------------------------------------- IP overflow
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_ip_overflow_ranks_like_the_model(va, dtype):
    dim, n = 8, 600
    rng = np.random.default_rng(11)
    mag = np.float32(3e38 / dim)
    raw = (rng.choice([-1.0, 1.0, 0.5, 1e-30], (n, dim)) * mag).astype(np.float32)
    raw[::7] = rng.standard_normal((raw[::7].shape[0], dim)).astype(np.float32)      # some ordinary rows
    vec = (rng.choice([-1.0, 1.0, 0.5], (12, dim)) * mag).astype(np.float32)
    vec[::5] = rng.standard_normal((vec[::5].shape[0], dim)).astype(np.float32)
    labels = rng.integers(0, 60, n).astype(np.uint32) * np.uint32(1_000_003)
    labels[:100] = 5 + np.arange(100, dtype=np.uint32)                                # documents of one row: M is that row's score
    model = MultivecModel(dim, dtype, "ip")
    lims = lims_of([1, 3, 8])
    with make_index(va, model, raw, labels) as ix:
        present, S = model.scores_multivec(vec, lims)
        assert np.isnan(S).any() and np.isinf(S).any() and np.isfinite(S).any(), "the overflow premise"
        for path in (PATH_AUTO, PATH_EXACT):
            ix.set_path(path)
            for k in (1, 7, 100):
                assert_same(ix.search_multivec(vec, k, lims=lims), model.rank(present, S, k), f"ip overflow path={path} k={k}")


# --------------------------------------------------------------------------------------------------------------- routes
def topical(rng, noise, dim=64, topics=200, docs=12):
    cent = rng.standard_normal((topics, dim)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    rows, labels = [], []
    for t in range(topics):
        for d in range(docs):
            m = int(rng.integers(1, 6))
            r = cent[t] + noise * rng.standard_normal((m, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
            rows.append(r / np.linalg.norm(r, axis=1, keepdims=True))
            labels += [t * docs + d + 1] * m
    raw = np.concatenate(rows).astype(np.float32)
    perm = rng.permutation(raw.shape[0])
    return cent, raw[perm], (np.asarray(labels, np.uint32) * np.uint32(2_654_435))[perm]


def topical_queries(rng, cent, noise, lens, dim=64):
    out = []
    for m in lens:
        t = int(rng.integers(0, cent.shape[0]))
        v = cent[t] + noise * rng.standard_normal((m, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
        out.append(v / np.linalg.norm(v, axis=1, keepdims=True))
    return np.concatenate(out).astype(np.float32), lims_of(lens)


LENS32 = [8, 33] * 16


@pytest.fixture(scope="module")
def topical_handle(va):
    rng = np.random.default_rng(2024)
    cent, raw, labels = topical(rng, 0.6)
    model = MultivecModel(64, "f32", "cosine")
    ix = make_index(va, model, raw, labels)
    vec, lims = topical_queries(rng, cent, 0.6, LENS32)
    present, S = model.scores_multivec(vec, lims)
    yield ix, model, vec, lims, present, S
    ix.close()


@pytest.mark.parametrize("k", [1, 5])
def test_route_certified(topical_handle, k):
    ix, model, vec, lims, present, S = topical_handle
    ok, k1 = model.routes(vec, lims, k, present, S)
    assert k1 == first_k(k, model.count) and ok.all(), f"premise: the model certifies {int(ok.sum())} of {ok.size} at k1 = {k1}"
    assert_same(ix.search_multivec(vec, k, lims=lims), model.rank(present, S, k), f"certified k={k}")
    mv, st = ix.last_multivec(), ix.last_stats()
    assert mv["certified_queries"] == ok.size and mv["dense_queries"] == 0 and mv["k1"] == k1, mv
    assert mv["candidate_labels"] >= ok.size * k and mv["candidate_rows"] >= mv["candidate_labels"]
    assert st["path"] != PATH_EXACT and st["nq"] == ok.size


def test_route_dense(va):
    rng = np.random.default_rng(99)
    cent, raw, labels = topical(rng, 20.0)                  # the row noise is far above the centroid: no structure
    model = MultivecModel(64, "f32", "cosine")
    vec, lims = topical_queries(rng, cent, 20.0, LENS32)
    with make_index(va, model, raw, labels) as ix:
        present, S = model.scores_multivec(vec, lims)
        for k in (1, 5):
            ok, _ = model.routes(vec, lims, k, present, S)
            assert not ok.any(), f"premise: the model certifies {int(ok.sum())} of {ok.size}"
            assert_same(ix.search_multivec(vec, k, lims=lims), model.rank(present, S, k), f"dense k={k}")
            mv, st = ix.last_multivec(), ix.last_stats()
            assert mv["dense_queries"] == ok.size and mv["certified_queries"] == 0, mv
            assert st["path"] == PATH_EXACT and st["fallback_queries"] >= ok.size


def test_route_mixed(topical_handle):
    ix, model, vec, lims, present, S = topical_handle
    k = 10
    # both kinds of query in one batch: the topical ones, and as many whose vectors are noise far above their centroid
    rng = np.random.default_rng(31)
    cent = rng.standard_normal((4, 64)).astype(np.float32)
    nv, nl = topical_queries(rng, cent / np.linalg.norm(cent, axis=1, keepdims=True), 20.0, [8, 33] * 8)
    half = int(lims[16])
    vec = np.concatenate([vec[:half], nv])
    lims = np.concatenate([lims[:17], nl[1:] + np.uint32(half)]).astype(np.uint32)
    present, S = model.scores_multivec(vec, lims)
    ok, k1 = model.routes(vec, lims, k, present, S)
    assert 0 < int(ok.sum()) < ok.size, f"premise: the model certifies {int(ok.sum())} of {ok.size}"
    assert_same(ix.search_multivec(vec, k, lims=lims), model.rank(present, S, k), "mixed k=10")
    mv = ix.last_multivec()
    assert mv["certified_queries"] + mv["dense_queries"] == ok.size
    assert mv["certified_queries"] == int(ok.sum()), (mv, ok.tolist())
    assert_same(device_form(ix, vec, lims, k), model.rank(present, S, k), "mixed k=10 device form")


# ------------------------------------------------------------------------------------------- more than one label pass
def test_candidate_route_over_several_label_passes(va):
    """The candidate route counts, lists and scores its labels in passes of kLabelGroupsPerPass = 4096 (label_plan.h).
    Every row its own document and 512 single-vector queries: their top-k1 lists name far more labels than one pass
    holds, so the counting loop and the list / score loop both run more than once."""
    n, dim, nq, k, per_pass = 16_384, 32, 512, 8, 4096
    rng = np.random.default_rng(4097)
    raw = rng.standard_normal((n, dim)).astype(np.float32)
    vec = rng.standard_normal((nq, dim)).astype(np.float32)
    labels = rng.permutation(n).astype(np.uint32) * np.uint32(3) + np.uint32(1)      # distinct, scattered, none of them 0
    lims = lims_of([1] * nq)
    model = MultivecModel(dim, "f32", "l2")
    with make_index(va, model, raw, labels) as ix:
        k1 = first_k(k, n)
        assert k1 == 40
        ids, _ = model._topk(np.arange(n), model._queries(vec), k1)                  # the exact lists of the first stage
        distinct = np.unique(labels[ids.astype(np.int64)]).size
        print("distinct candidate labels", distinct)
        assert distinct > per_pass, f"premise: {distinct} distinct labels in the top-{k1} lists"
        assert_same(ix.search_multivec(vec, k, lims=lims), model.search_multivec(vec, lims, k), "several label passes")
        mv, st = ix.last_multivec(), ix.last_stats()
        print(mv, st)
        assert mv["candidate_labels"] > 0 and mv["certified_queries"] + mv["dense_queries"] == nq and mv["k1"] == k1, mv
        # no list holds a NaN, 40 candidate rows are not too broad and 512 * 40 score slots fit (multivec_plan.h): every
        # query stays on the candidate route up to the certificate, so all `distinct` labels are listed and scored
        assert mv["candidate_labels"] == nq * k1 and mv["candidate_rows"] == nq * k1, mv
