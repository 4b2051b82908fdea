"""The inputs of tests/test_gpu_certificate.py do aim at the certificate's error bound (no GPU: fp64 numpy and the CPU
oracle on the PREPARED values, i.e. what the kernels see).  A fixture that quietly became benign would keep the GPU
tests green while testing nothing: these checks fail instead."""
import numpy as np
import pytest

import certificate_fixtures as F
from support import DT, ME


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [768, 3072])
def test_cancel_sums_climb_and_come_back(oracle, dtype, metric, dim):
    raw, rq = F.cancel(512, 16, dim)
    x = oracle.prepare(raw, DT[dtype], ME[metric]).astype(np.float64)
    q = oracle.prepare(rq, DT[dtype], ME[metric]).astype(np.float64)
    absdot = np.abs(q) @ np.abs(x).T
    ratio = absdot / np.maximum(np.abs(q @ x.T), 1e-300)
    assert np.mean(ratio >= 100.0) >= 0.9, np.quantile(ratio, [0.01, 0.1, 0.5])
    # sum |q_j x_j| is the bound's |q||x| up to a small factor (the bound's worst case), and the left-to-right partial
    # sum climbs to about half of it before it comes back
    norms = np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None, :]
    assert np.min(absdot / norms) >= 0.8
    peak = np.abs(np.cumsum(q[:, None, :] * x[None, :, :], axis=2)).max(axis=2)
    assert np.min(peak / norms) >= 0.4


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_range_rows_span_2_to_the_20(oracle, dtype, metric):
    raw, rq = F.range_(512, 16, 768, metric)
    for v in (raw, rq):
        p = np.abs(oracle.prepare(v, DT[dtype], ME[metric]).astype(np.float64))
        assert (p > 0).all()
        assert np.min(p.max(axis=1) / p.min(axis=1)) >= 2.0 ** 20 * 0.99
    if metric == "l2":
        scale = np.abs(raw).max(axis=1)
        assert scale.min() < 1e-2 and scale.max() > 1e2       # row scales from ~1e-3 to ~1e3


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [768, 3072])
def test_split_worst_reaches_the_representation_term(oracle, metric, dim):
    """The exact error of the split product qh.xh + ql.xh + qh.xl against q.x, over the prepared fp32 values, is at
    least 1/8 of the bound's representation term 3.1 * 2^-16 |q||x| for every pair (a coherent construction gets ~1/4;
    random data ~1/300)."""
    raw, rq = F.split_worst(256, 16, dim, metric)
    x = oracle.prepare(raw, 0, ME[metric])
    q = oracle.prepare(rq, 0, ME[metric])
    if metric == "cosine":   # built with norm 1: normalising changed no bit, the pattern is what the kernels see
        assert np.array_equal(x.view(np.uint32), raw.view(np.uint32))
        assert np.array_equal(q.view(np.uint32), rq.view(np.uint32))
    xh, xl = (a.astype(np.float64) for a in F.split_planes(x))
    qh, ql = (a.astype(np.float64) for a in F.split_planes(q))
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    err = q64 @ x64.T - (qh @ xh.T + ql @ xh.T + qh @ xl.T)   # bf16 x bf16 and fp32 x fp32 products are exact in fp64
    term = F.SPLIT_REPR * np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(x64, axis=1)[None, :]
    assert np.min(np.abs(err) / term) >= 1.0 / 8.0, np.quantile(np.abs(err) / term, [0.0, 0.5])
    assert (err > 0).all()      # one sign: the terms add up


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("k", [10, 100])
def test_near_ties_put_the_kth_place_in_a_cluster(oracle, dtype, metric, k):
    """At least k + 1 canonical scores within the batched scan's bound of the k-th -- most of the cluster within a tenth
    of it -- so no certificate can hold and the band pass has to answer."""
    dim = 128
    raw, rq, nc = F.near_ties(20000, 8, dim, metric, dtype, k)
    assert nc == 8
    x = oracle.prepare(raw, DT[dtype], ME[metric])
    q = oracle.prepare(rq, DT[dtype], ME[metric])
    m = 3 * k + 8
    _, sc = oracle.scan_topk(x, q, m, ME[metric], threads=8)
    xn = np.sqrt((x.astype(np.float64) ** 2).sum(1)).max()
    for i in range(nc):
        qn = np.sqrt((q[i].astype(np.float64) ** 2).sum())
        eps = F.mfma_eps(dim, metric, False, qn, xn)
        d = np.abs(sc[i].astype(np.float64) - float(sc[i, k - 1]))
        assert np.sum(d <= eps) >= k + 1, (i, d[:k + 2], eps)
        assert np.sum(d <= eps / 10) >= 2 * k, (i, np.sort(d)[: 2 * k + 1], eps)


@pytest.mark.parametrize("dim", [768, 3072])
def test_offset_cluster_cancels_in_the_norm_expansion(oracle, dim):
    raw, rq = F.offset_cluster(512, 16, dim)
    x = raw.astype(np.float64)
    q = rq.astype(np.float64)
    d2 = ((q[:, None, :] - x[None, :, :]) ** 2).sum(2)
    n2 = (q * q).sum(1)[:, None] + (x * x).sum(1)[None, :]
    assert np.max(d2 / n2) <= 1e-5                    # |q|^2 + |x|^2 - 2 q.x gives away > 5 decimal digits
    assert np.min(np.linalg.norm(x, axis=1)) >= 900 * np.max(np.linalg.norm(x - x.mean(0), axis=1))
