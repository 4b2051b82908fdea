"""Split pass for fp32 corpora (default while memory allows; VROD_F32_SPLIT=0 / 1 at handle creation
switch it off / force it): the batched fast pass runs on the bf16 matrix cores over [hi | lo] planes of the fp32 rows (q.x ~ hi.hi + hi.lo +
lo.hi).  Only the fast pass changes: candidates are re-scored canonically and certified against a
bound that covers the representation error, so ids and score bits must still be the oracle's.
"""
import os

import numpy as np
import pytest

from support import ME, va, bits  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture()
def split_env():
    old = os.environ.get("VROD_F32_SPLIT")
    os.environ["VROD_F32_SPLIT"] = "1"     # read when a handle is created
    yield
    if old is None:
        del os.environ["VROD_F32_SPLIT"]
    else:
        os.environ["VROD_F32_SPLIT"] = old


@pytest.mark.parametrize("metric", ["cosine", "l2"])
# (batches of <= 32 queries take the skinny form of the split pass where [hi | lo] of the queries fit
#  in LDS: 16 queries at d = 1536, 32 at d = 768)
@pytest.mark.parametrize("dim,nq,k", [(100, 40, 10), (129, 300, 100), (768, 64, 10), (64, 13, 1000),
                                      (768, 13, 10), (768, 30, 10), (300, 17, 50), (1536, 16, 10), (1536, 20, 10)])
def test_split_pass_is_bit_exact(va, oracle, split_env, metric, dim, nq, k):
    rng = np.random.default_rng(dim + nq)
    n = 30011
    raw = (rng.standard_normal((n, dim)) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)
    rq = rng.standard_normal((nq, dim)).astype(np.float32)
    with va.Index(dim, "f32", metric) as ix:
        ix.add(raw[:20000])
        ids0, sc0 = ix.search(rq, k)              # planes built for 20000 rows
        ix.add(raw[20000:])                       # ... and extended lazily at the next batched search
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
    assert st["path"] == 2 and st["split_pass"] == 1, "AUTO must route a batch of >= 13 queries to the MFMA (split) pass"
    assert st["kprime"] == min(n, k + max(32, k // 2))
    oi, osc = oracle.search(raw, rq, k, 0, ME[metric])
    assert np.array_equal(ids, oi), np.argwhere(ids != oi)[:5]
    assert np.array_equal(bits(sc), bits(osc))
    o0, s0 = oracle.search(raw[:20000], rq, k, 0, ME[metric])
    assert np.array_equal(ids0, o0) and np.array_equal(bits(sc0), bits(s0))
    assert st["max_fast_err"] <= st["eps_bound"], st
    if metric == "cosine":                          # (L2 over rows of very different norms: the bound scales with
        assert st["fallback_queries"] <= nq // 10, st   #  the largest norm and many queries take the exact path)


def test_split_is_the_default_but_not_for_small_batches_or_when_switched_off(va, oracle):
    from conftest import f32_split
    raw = oracle.synth_rows(1, 0, 20000, 96)
    rq8 = oracle.synth_rows(2, 0, 8, 96)
    rq = oracle.synth_rows(2, 0, 40, 96)
    oi, osc = oracle.search(raw, rq, 10, 0, 0)
    with f32_split(None), va.Index(96, "f32", "cosine") as ix:
        ix.add(raw)
        ix.search(rq8[:4], 10)
        assert ix.last_stats()["path"] == 1          # 4 queries: the stream scan, split or not
        assert ix.last_stats()["split_pass"] == 0
        i8, s8 = ix.search(rq8, 10)                  # 5-32 queries: the skinny form of the split pass
        assert ix.last_stats()["path"] == 2 and ix.last_stats()["split_pass"] == 1
        o8, os8 = oracle.search(raw, rq8, 10, 0, 0)
        assert np.array_equal(i8, o8) and np.array_equal(bits(s8), bits(os8))
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
        assert st["path"] == 2 and st["split_pass"] == 1 and st["kprime"] == 10 + 32
        assert np.array_equal(ids, oi) and np.array_equal(bits(sc), bits(osc))
    with f32_split("0"), va.Index(96, "f32", "cosine") as ix:
        ix.add(raw)
        ids, sc = ix.search(rq, 10)
        st = ix.last_stats()
    assert st["path"] == 2 and st["split_pass"] == 0 and st["kprime"] == 10 + 8    # the fp32 MFMA pass and its k' (cosine: margin 8)
    assert np.array_equal(ids, oi) and np.array_equal(bits(sc), bits(osc))
    with f32_split(None), va.Index(96, "bf16", "cosine") as ix:      # bf16 handles have no planes
        ix.add(raw)
        ix.search(rq, 10)
        assert ix.last_stats()["split_pass"] == 0


def test_a_corpus_the_split_bound_cannot_certify_is_resolved_by_the_band_pass(va, oracle):
    """Rows whose squared distances from the query climb by 3e-6 of the largest one per rank: the
    gap k .. k' is wider than the fp32 pass's bound (3.2e-5 of it over 16 ranks) and narrower than
    the split pass's (1.4e-4 over 32), so every query fails the split certificate.  Round 2 answered
    that by switching the handle back to the fp32 pass after two such searches; the heuristic now counts
    what is left AFTER the band pass (one more shared scan on the bf16 matrix cores resolves all of
    them: cheaper than the fp32 pass at 1/16 of the matrix rate), so the split pass stays.  Forced (=1)
    likewise.  Results are the oracle's bits throughout."""
    from conftest import f32_split
    rng = np.random.default_rng(5)
    n, dim, nq, k = 30000, 128, 48, 10
    u = rng.standard_normal((n, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d2 = 0.9 + 3e-6 * rng.permutation(n)
    raw = (u * np.sqrt(d2)[:, None]).astype(np.float32)
    rq = np.zeros((nq, dim), dtype=np.float32)
    oi, osc = oracle.search(raw, rq, k, 0, 1)
    seen = []
    with f32_split(None), va.Index(dim, "f32", "l2") as ix:
        ix.add(raw)
        for _ in range(4):
            ids, sc = ix.search(rq, k)
            st = ix.last_stats()
            seen.append((st["split_pass"], st["fallback_queries"], st["band_queries"]))
            assert np.array_equal(ids, oi) and np.array_equal(bits(sc), bits(osc))
            assert 0 < st["max_fast_err"] <= st["eps_bound"], st
    assert seen[0][0] == 1 and seen[0][1] * 8 > nq, f"the case is meant to defeat the split bound: {seen}"
    assert all(s[0] == 1 and s[2] == s[1] for s in seen), f"every failed certificate is resolved by the band pass, the split pass stays: {seen}"
    with f32_split("1"), va.Index(dim, "f32", "l2") as ix:
        ix.add(raw)
        for _ in range(3):
            ids, sc = ix.search(rq, k)
            assert ix.last_stats()["split_pass"] == 1
            assert np.array_equal(ids, oi) and np.array_equal(bits(sc), bits(osc))
