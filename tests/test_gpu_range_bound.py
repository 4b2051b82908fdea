"""The range search's superset premise on the inputs built to reach the error bound, for every fast kernel.

vrod_range_search has no certificate: it widens the caller's threshold by the bound (search_plan.h
range_fast_threshold), runs one filtered launch, and re-scores only what that launch listed.  A row whose fast score
falls outside the widened threshold is lost without a trace (max_fast_err is measured over the listed rows only).
Only lims, ids and score bits equal to the oracle's -- on inputs where rows do lie within one bound of the threshold,
which tests/test_range_bound_cases.py checks on the CPU for these same cases -- can show that.  Cases, thresholds and
the band condition: tests/range_bound_cases.py."""
import numpy as np
import pytest

import range_bound_cases as R
from support import PATH_MFMA, va, bits  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_range_search_on_the_bound_families(va, oracle, case):
    from conftest import f32_split
    name, dim, metric, family, n = case
    dtype, path, nq, mode, split_pass, _ = R.KERNELS[name]
    c = R.build(oracle, case)
    print(R.report(case, c))
    assert c["share"] >= R.MIN_QUERY_SHARE, R.report(case, c)       # checked before the GPU is asked; not a tolerance
    with f32_split(mode), va.Index(dim, dtype, metric) as ix:
        ix.add(c["raw"])
        ix.set_path(path)
        lims, ids, sc = ix.range_search(c["rq"], c["thr"])
        st = ix.last_stats()
    what = f"{name} {dtype}/{metric} d={dim} {family} n={n}"
    print(what, {k: st[k] for k in ("path", "split_pass", "kprime", "scan_launches", "fallback_queries", "max_fast_err", "eps_bound")})
    ol, oi, osc = c["want"]
    assert np.array_equal(lims, ol), f"{what}: lims differ at queries {np.argwhere(np.diff(lims.astype(np.int64)) != np.diff(ol.astype(np.int64)))[:8].ravel()}"
    assert np.array_equal(ids, oi), f"{what}: ids differ at {np.argwhere(ids != oi)[:5].ravel()}"
    assert np.array_equal(bits(sc), bits(osc)), f"{what}: score bits differ"
    assert st["path"] == PATH_MFMA and st["split_pass"] == split_pass, (what, st)
    assert st["fallback_queries"] == 0, (what, st)                  # every bound here is finite: no canonical route
    assert np.isfinite(st["eps_bound"]) and st["max_fast_err"] <= st["eps_bound"], \
        f"{what}: max_fast_err / eps_bound = {st['max_fast_err'] / st['eps_bound']:.3g}"
    # the restated bound is the library's (fp32 against fp64 arithmetic)
    assert abs(st["eps_bound"] - c["eps"]) <= 1e-3 * c["eps"], (what, st["eps_bound"], c["eps"])
    if family == "cancel":
        assert st["max_fast_err"] > 0, (what, st)
    if family == "offset_cluster":
        assert st["scan_launches"] > 1, (what, st)                  # the lists overflowed: the rows were redone in pieces
