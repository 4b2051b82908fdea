"""The certificate's premise checked where it is weakest: the fast score of EVERY row is within eps_bound of its
canonical score, on inputs built to reach the bound (tests/certificate_fixtures.py; that they do is
tests/test_certificate_fixtures.py), for every fast kernel.

Every-row check: N <= VROD_MAX_K rows and k = N.  Every row is then a candidate (k' = N), the canonical re-score covers
them all, and max_fast_err -- measured on the device over the candidates -- is the maximum over the whole corpus.
Staged check: the same families at 300k rows, so that the sample pass, the thresholds between stages and the band pass
run on them."""
import numpy as np
import pytest

import certificate_fixtures as F
from support import DT, ME, va, bits  # noqa: F401

pytestmark = pytest.mark.gpu

KERNELS = F.KERNELS     # which kernel a batch reaches: certificate_fixtures.py
N_ALL = 2048     # <= VROD_MAX_K, and k' = N fits the split pass's k + max(32, k / 2) <= 4096


def _families(dtype, metric):
    fam = ["cancel", "range"]
    if dtype == "f32":
        fam.append("split_worst")
    if metric == "l2":
        fam.append("offset_cluster")
    return fam


def _cases():
    out = []
    for name, (dtype, path, nq, mode, sp, dims) in KERNELS.items():
        for dim in dims:
            for metric in ("cosine", "l2"):
                for fam in _families(dtype, metric):
                    out.append(pytest.param(name, dim, metric, fam, id=f"{name}-{dim}-{metric}-{fam}"))
    return out


def _search(va, raw, rq, k, dtype, metric, path, mode):
    from conftest import f32_split
    with f32_split(mode), va.Index(raw.shape[1], dtype, metric) as ix:
        ix.add(raw)
        ix.set_path(path)
        ids, sc = ix.search(rq, k)
        return ids, sc, ix.last_stats()


@pytest.mark.parametrize("name,dim,metric,family", _cases())
def test_every_row_is_within_the_bound(va, oracle, name, dim, metric, family):
    dtype, path, nq, mode, split_pass, _ = KERNELS[name]
    raw, rq = F.make(family, N_ALL, nq, dim, metric, dtype, seed=dim)
    ids, sc, st = _search(va, raw, rq, N_ALL, dtype, metric, path, mode)
    oi, osc = oracle.search(raw, rq, N_ALL, DT[dtype], ME[metric], threads=16)
    what = f"{name} {dtype}/{metric} d={dim} {family}"
    assert st["path"] == path and st["split_pass"] == split_pass, (what, st)
    assert st["kprime"] == N_ALL, (what, st)          # every row re-scored: max_fast_err covers the corpus
    assert np.array_equal(ids, oi), f"{what}: ids differ at {np.argwhere(ids != oi)[:5]}"
    assert np.array_equal(bits(sc), bits(osc)), f"{what}: score bits differ"
    ratio = st["max_fast_err"] / st["eps_bound"]
    print(f"CERT_RATIO {name} {metric} {dim} {family} {st['max_fast_err']:.3e} {st['eps_bound']:.3e} {ratio:.3e}")
    assert np.isfinite(st["eps_bound"]) and st["max_fast_err"] <= st["eps_bound"], \
        f"{what}: max_fast_err / eps_bound = {ratio:.3g} ({st['max_fast_err']:.3e} / {st['eps_bound']:.3e})"
    if family == "cancel":
        # the statistic is live: order-dependent rounding of a cancelling sum cannot come out exact on every row
        assert st["max_fast_err"] > 0, (what, st)


STAGED = [
    # family, dtype, metric, VROD_F32_SPLIT
    ("cancel", "bf16", "cosine", None),
    ("range", "bf16", "l2", None),
    ("split_worst", "f32", "l2", "1"),
    ("near_ties", "bf16", "cosine", None),
    ("offset_cluster", "f32", "l2", "1"),
]


@pytest.mark.parametrize("k,nq", [(10, 1024), (100, 40)])
@pytest.mark.parametrize("family,dtype,metric,mode", STAGED, ids=[s[0] for s in STAGED])
def test_staged_search_on_the_bound_families(va, oracle, family, dtype, metric, mode, k, nq):
    """300k x 128: the dense sample pass, filtered stages with thresholds in between, and -- for the near-ties -- the
    band pass.  Bits = the oracle's; the bound holds wherever it is finite (on the offset cluster the L2 bound is far
    wider than the distances: the certificates refuse and the band / exact path answers, exactly all the same)."""
    n, dim = 300_000, 128
    raw, rq = F.make(family, n, nq, dim, metric, dtype, k=k, seed=7)
    ids, sc, st = _search(va, raw, rq, k, dtype, metric, 2, mode)
    oi, osc = oracle.search(raw, rq, k, DT[dtype], ME[metric], threads=16)
    what = f"{family} {dtype}/{metric} k={k} nq={nq}"
    assert st["path"] == 2 and st["scan_launches"] >= 3, (what, st)
    assert st["split_pass"] == (1 if mode == "1" else 0), (what, st)
    assert np.array_equal(ids, oi), f"{what}: ids differ at {np.argwhere(ids != oi)[:5]}"
    assert np.array_equal(bits(sc), bits(osc)), f"{what}: score bits differ"
    if np.isfinite(st["eps_bound"]):
        ratio = st["max_fast_err"] / st["eps_bound"]
        print(f"CERT_RATIO_STAGED {family} {dtype} {metric} k={k} nq={nq} {ratio:.3e} fb={st['fallback_queries']} band={st['band_queries']}")
        assert st["max_fast_err"] <= st["eps_bound"], f"{what}: max_fast_err / eps_bound = {ratio:.3g}"
    if family == "near_ties":
        assert st["band_queries"] > 0, (what, st)
