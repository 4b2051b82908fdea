"""Seeded inputs aimed at the certificate's error bound, shared by the CPU test that checks they do
aim at it (tests/test_certificate_fixtures.py) and the GPU tests that run every fast kernel on them
(tests/test_gpu_certificate.py).  Every generator returns raw fp32 (corpus, queries); the handle prepares them as usual.

  cancel          dot products that climb to about half of |q||x| and come back: score ~ 0, sum |q_j x_j| ~ |q||x|
  range           |x_j| log-uniform over 2^20 inside every row (L2: row scales 1e-3 .. 1e3 as well)
  split_worst     fp32 elements whose bf16 split x = hi + lo + r has lo and r near their maxima and of one sign, queries
                  alike: the dropped terms of qh.xh + ql.xh + qh.xl add coherently (cosine rows are built with norm 1
                  to well under an fp32 ulp, so that normalising them changes no bit)
  near_ties       per query a cluster of rows (a base row and one-ulp perturbations of it) whose canonical scores lie
                  within a tenth of the bound of each other: the k-th place sits inside the cluster
  offset_cluster  L2: rows and queries = c + noise with |c| ~ 1e3 |noise|: |q|^2 + |x|^2 - 2 q.x cancels
"""
import numpy as np

U = 2.0 ** -24
SPLIT_REPR = 3.1 * 2.0 ** -16          # the split pass's representation term (search_plan.h)


# Which kernel a batch reaches, by the dispatcher's rule (search_plan.h route -- checked on the CPU by
# test_search_plan.py --, kernels_mfma.hip launch_scan_mfma, kernels_mfma_skinny.hip mfma_skinny_max_queries):
#   stream       path STREAM forced, <= 4 queries: kernels_stream.hip, one pass per 8 queries
#   skinny       bf16 rows, path MFMA, 5..64 queries, the queries fit in LDS (64-query form at d = 768; not at d = 3072)
#   w4           bf16 rows, path MFMA, > 64 queries: the 4-wave kernel
#   w4-split     fp32 rows, VROD_F32_SPLIT=1, > 32 queries: the 4-wave kernel's SPLIT form over the [hi | lo] planes
#   skinny-split fp32 rows, VROD_F32_SPLIT=1, <= 32 queries whose [hi | lo] fit in LDS (d = 768; not at d = 3072)
#   phased       fp32 rows, VROD_F32_SPLIT=0, path MFMA: the 8-wave fp32 matrix-core kernel
KERNELS = {
    # name: (dtype, path, queries, VROD_F32_SPLIT, split_pass, dims)
    "stream-f32": ("f32", 1, 4, "0", 0, (768, 3072)),
    "stream-bf16": ("bf16", 1, 4, None, 0, (768, 3072)),
    "skinny": ("bf16", 2, 33, None, 0, (768,)),
    "w4": ("bf16", 2, 100, None, 0, (768, 3072)),
    "w4-split": ("f32", 2, 100, "1", 1, (768, 3072)),
    "skinny-split": ("f32", 2, 20, "1", 1, (768,)),
    "phased": ("f32", 2, 100, "0", 0, (768, 3072)),
}


def bf16_rne(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return (r.astype(np.uint32) << np.uint32(16)).view(np.float32)


def split_planes(a):
    """The library's split of fp32 values (split_rows_kernel): hi = bf16_rne(x), lo = bf16_rne(x - hi)."""
    a = np.asarray(a, dtype=np.float32)
    hi = bf16_rne(a)
    lo = bf16_rne((a - hi).astype(np.float32))
    return hi, lo


def mfma_eps(dim, metric, split, qn, xn):
    """The batched scan's certificate bound for query norm qn and largest row norm xn (search_plan.h fast_bound and
    eps_bound; test_search_plan.py checks that they agree)."""
    if split:
        c = 4.1 * (3 * dim + (0 if metric == "cosine" else 4)) * U + SPLIT_REPR
    else:
        c = 4.0 * (dim + (0 if metric == "cosine" else 4)) * U
    return c * qn * xn if metric == "cosine" else c * (qn + xn) ** 2


def cancel(n, nq, dim, seed=1):
    rng = np.random.default_rng(seed)
    h = dim // 2
    prof = rng.uniform(0.5, 1.5, h)                      # a positive magnitude profile every vector follows
    sig = rng.choice([-1.0, 1.0], h)                     # column signs, common to all: products keep their sign

    def vecs(m, second_sign):
        first = prof * np.exp(0.25 * rng.standard_normal((m, h)))
        second = first * (1.0 + 0.02 * rng.standard_normal((m, h)))
        out = np.zeros((m, dim))
        out[:, :h] = first * sig
        out[:, h:2 * h] = second_sign * second * sig
        return out.astype(np.float32)

    # q = (u, u'), x = (w, -w'): the first half adds ~ u.w ~ |q||x| / 2, the second half takes it back
    return vecs(n, -1.0), vecs(nq, 1.0)


def range_(n, nq, dim, metric, seed=2):
    rng = np.random.default_rng(seed)

    def vecs(m):
        e = rng.uniform(0.0, 20.0, (m, dim))
        cols = np.argsort(rng.random((m, dim)), axis=1)[:, :2]
        np.put_along_axis(e, cols[:, :1], 0.0, axis=1)   # every row spans exactly 2^20
        np.put_along_axis(e, cols[:, 1:], 20.0, axis=1)
        v = rng.choice([-1.0, 1.0], (m, dim)) * np.exp2(-e)
        if metric == "l2":
            v *= 10.0 ** rng.uniform(-3.0, 3.0, (m, 1))
        return v.astype(np.float32)

    return vecs(n), vecs(nq)


def _split_worst_values(rng, shape, exps):
    # significand 1.hhhhhhh 0 11111111 0111111 (24 bits): hi = 1.hhhhhhh (bit 15 = 0 rounds down), lo = the eight ones
    # (bit 6 = 0 rounds down again: lo at its largest, below hi's half ulp), r = 0111111 (just under half of lo's ulp)
    h = rng.integers(0, 64, shape).astype(np.int64)
    sig = (1 << 23) | (h << 16) | (0xFF << 7) | 0x3F
    return np.ldexp(sig.astype(np.float64), exps - 23)


def split_worst(n, nq, dim, metric, seed=3):
    rng = np.random.default_rng(seed)
    sig = rng.choice([-1.0, 1.0], dim)                     # column signs common to all vectors: q_j x_j > 0
    base = rng.integers(-2, 1, dim)                        # a common exponent profile: |q_j| ~ |x_j|

    def vecs(m):
        exps = base[None, :] + rng.integers(0, 2, (m, dim))
        v = _split_worst_values(rng, (m, dim), exps)
        if metric == "cosine":
            v = _unit_rows(v, dim)
        return (v * sig).astype(np.float32)

    return vecs(n), vecs(nq)


def _unit_rows(v, dim):
    """Rows of pattern values scaled (by powers of two, bit pattern kept) to a squared norm just under 1, the first two
    columns replaced by fix-up elements that bring it to 1 within ~2^-40: the library's normalisation (x / |x| in fp64,
    rounded to fp32) then gives back every element unchanged."""
    v = v.copy()
    v[:, :2] = 0.0
    s = (v * v).sum(axis=1)
    v *= np.exp2(-np.ceil(np.log2(s) / 2.0))[:, None]                # squared norm in [1/4, 1)
    rng = np.random.default_rng(dim)
    for _ in range(2):   # double the elements of a random prefix of the columns while the squared norm stays below 1
        gap = 1.0 - (v * v).sum(axis=1)
        perm = np.argsort(rng.random(v.shape), axis=1)
        add = np.take_along_axis(3.0 * v * v, perm, axis=1)
        grow = np.cumsum(add, axis=1) <= (gap - 2.0 ** -12)[:, None]
        f = np.ones_like(v)
        np.put_along_axis(f, perm, np.where(grow, 2.0, 1.0), axis=1)
        f[:, :2] = 1.0
        v *= f
    gap = 1.0 - (v * v).sum(axis=1)
    f1 = np.sqrt(gap).astype(np.float32).astype(np.float64)
    over = f1 * f1 > gap
    f1[over] = np.nextafter(f1[over].astype(np.float32), np.float32(0)).astype(np.float64)
    f2 = np.sqrt(np.maximum(gap - f1 * f1, 0.0)).astype(np.float32).astype(np.float64)
    v[:, 0], v[:, 1] = f1, f2
    return v


def _one_ulp(x, dtype):
    """x moved by one unit in the last place of the handle's element type (away from zero)."""
    x = np.float32(x)
    if dtype == "bf16":
        b = bf16_rne(np.array([x]))[0]
        return np.float32((np.array([b]).view(np.uint32) + np.uint32(1 << 16)).view(np.float32)[0])
    return np.nextafter(x, np.float32(np.copysign(np.inf, x)))


def near_ties(n, nq, dim, metric, dtype, k, clusters=None, seed=4):
    """The first `clusters` queries (default: all that fit) each get 3k + 8 rows: a base row and copies of it with one
    element moved by one ulp, that element one of the 16 whose move changes the score least.  The query is the base
    row plus a little noise; the rest of the corpus is random and far away."""
    rng = np.random.default_rng(seed)
    m = 3 * k + 8
    nc = min(nq, n // (2 * m)) if clusters is None else clusters
    corpus = rng.standard_normal((n, dim)).astype(np.float32)
    if metric == "cosine":
        corpus[:, 0] = -np.abs(corpus[:, 0]) - 4.0         # far from every cluster (whose column 0 is large and > 0)
    else:
        corpus += 6.0
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    base = rng.standard_normal((nc, dim))
    base[:, 0] = np.abs(base[:, 0]) + 4.0
    if dtype == "bf16":
        base = bf16_rne(base.astype(np.float32)).astype(np.float64)
    rows = rng.permutation(n)[: nc * m].reshape(nc, m) if nc else np.zeros((0, m), dtype=np.int64)
    for c in range(nc):
        b = base[c].astype(np.float32)
        q = (b + 1e-3 * rng.standard_normal(dim)).astype(np.float32)
        queries[c] = q
        impact = np.abs(q) if metric == "cosine" else np.abs(b - q) + 1e-3
        low = np.argsort(impact * np.abs(b))[:16]
        corpus[rows[c, 0]] = b
        for i, r in enumerate(rows[c, 1:]):
            x = b.copy()
            j = low[i % 16]
            x[j] = _one_ulp(x[j], dtype) if (i // 16) % 2 == 0 else -_one_ulp(-x[j], dtype)
            corpus[r] = x
    return corpus, queries, nc


def offset_cluster(n, nq, dim, seed=5):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(dim)
    c *= 1e3 / np.linalg.norm(c)
    noise = lambda m: rng.standard_normal((m, dim)) / np.sqrt(dim)   # |noise| ~ 1, |c| = 1e3
    return (c + noise(n)).astype(np.float32), (c + noise(nq)).astype(np.float32)


FAMILIES = ("cancel", "range", "split_worst", "near_ties", "offset_cluster")


def make(family, n, nq, dim, metric, dtype, k=10, seed=0):
    """(corpus, queries) of one family; near_ties also needs the handle's dtype and k."""
    if family == "cancel":
        return cancel(n, nq, dim, seed + 1)
    if family == "range":
        return range_(n, nq, dim, metric, seed + 2)
    if family == "split_worst":
        return split_worst(n, nq, dim, metric, seed + 3)
    if family == "near_ties":
        c, q, _ = near_ties(n, nq, dim, metric, dtype, k, seed=seed + 4)
        return c, q
    if family == "offset_cluster":
        assert metric == "l2"
        return offset_cluster(n, nq, dim, seed + 5)
    raise ValueError(family)
