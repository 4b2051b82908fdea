"""The cases of tests/test_gpu_range_bound.py do put their thresholds where the fast pass's error can matter (no GPU:
the oracle's canonical scores and certificate_fixtures.mfma_eps).  A case whose thresholds sat in empty stretches of the
score distribution would keep the GPU test green whatever bound the range search widened by: this check fails instead."""
import numpy as np
import pytest

import range_bound_cases as R


@pytest.mark.parametrize("case", R.cases(), ids=R.case_id)
def test_thresholds_sit_inside_the_band(oracle, case):
    c = R.build(oracle, case)
    print(R.report(case, c))
    name, dim, metric, family, n = case
    nq = R.KERNELS[name][2]
    assert c["thr"].shape == (nq,) and np.isfinite(c["thr"]).all()
    assert c["share"] >= R.MIN_QUERY_SHARE, R.report(case, c)
    counts = np.diff(c["want"][0].astype(np.int64))
    assert (counts[0::3] >= 1).all()                  # "exactly a row's score": that row qualifies
    if family == "near_ties":                         # the cluster straddles the boundary: some members in, some out
        m, nc = 3 * R.NEAR_TIES_K + 8, c["nc"]        # (a cluster whose members all tie on one score cannot)
        assert nc >= 1 and (counts[:nc] <= m).all()
        assert np.mean((counts[:nc] >= 1) & (counts[:nc] < m)) >= R.MIN_QUERY_SHARE, counts[:nc]
    if family == "offset_cluster":                    # the bound is wider than the whole score distribution
        assert (c["n_in"] + c["n_out"] == n).all()
    if n == R.N_LARGE and family != "near_ties":      # thresholds among the best rows: the answers stay small
        assert counts.max() <= R.LARGE_BEST + 64, counts.max()


def test_every_kernel_and_family_is_covered():
    cs = R.cases()
    assert len(set(cs)) == len(cs)
    for name, (dtype, _, _, _, _, dims) in R.KERNELS.items():
        for dim in dims + (R.DIM_LARGE,):
            fams = {c[3] for c in cs if c[0] == name and c[1] == dim}
            want = {"cancel", "range", "offset_cluster"} | ({"split_worst"} if dtype == "f32" else set())
            if dtype == "bf16" or dim == R.DIM_LARGE:          # where the clusters spread over score levels
                want.add("near_ties")
            assert fams == want, (name, dim, fams)
            ties = {c[2] for c in cs if c[0] == name and c[1] == dim and c[3] == "near_ties"}
            assert ties == ({"l2", "cosine"} if dtype == "bf16" and dim == R.DIM_LARGE else {"l2"} if "near_ties" in want else set()), (name, dim, ties)
        for fam in ("cancel", "range"):
            assert any(c[0] == name and c[2] == "ip" and c[3] == fam for c in cs), (name, fam)
    assert "stream-f32" not in R.KERNELS and len(R.KERNELS) == 5
