"""GPU tests of the inner-product metric (VROD_METRIC_IP = 2) against the CPU oracle.

The oracle needs no IP mode of its own: an IP search is `prepare(raw, dtype, METRIC_L2)` (stored as
given, bf16-rounded on BF16 handles) followed by `scan_topk(..., METRIC_COSINE)` (the canonical dot,
higher is better).  Bar: ids and score bits equal to that composition on every path and dtype; a
NaN score (an overflowing dot product: +inf + -inf) only has to be NaN, its payload is the
platform's.  Wherever the certificate's bound is finite and the path is not EXACT, the observed
|fast - canonical| must lie inside it.
"""
import os
import subprocess

import numpy as np
import pytest

from support import DT, METRIC_COSINE, METRIC_L2, THREADS, va, bits, assert_same, check_bound  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VROD = os.path.join(ROOT, "vrod_amd", "vrod")


def oracle_ip(O, raw, rq, k, dtype, id_offset=0):
    pc = O.prepare(raw, DT[dtype], METRIC_L2, threads=THREADS)
    pq = O.prepare(rq, DT[dtype], METRIC_L2, threads=THREADS)
    return O.scan_topk(pc, pq, k, METRIC_COSINE, id_offset=id_offset, threads=THREADS)


def run_case(va, O, raw, rq, k, dtype, path, split=None, expect=None):
    from conftest import f32_split
    oi, osc = expect if expect is not None else oracle_ip(O, raw, rq, k, dtype)
    with f32_split(split), va.Index(raw.shape[1], dtype, "ip") as ix:
        ix.add(raw)
        ix.set_path(path)
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
    what = f"ip/{dtype}/path{path}/split={split}/nq={rq.shape[0]}/k={k}"
    assert_same(ids, sc, oi, osc, what)
    check_bound(st, what)
    if split == "0":
        assert st["split_pass"] == 0
    if split == "1" and st["path"] == 2:
        assert st["split_pass"] == 1
    return ids, sc, st


def skewed(rng, n, d, offset=6.0, lo=-3.0, hi=3.0):
    """Gaussian rows around a common direction (e_0 * offset), each scaled by exp(U(lo, hi))."""
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[:, 0] += offset
    return (x * np.exp(rng.uniform(lo, hi, (n, 1)))).astype(np.float32)


def skewed_queries(rng, nq, d):
    """Half random, half aimed against the corpus's common direction: every score of those is negative."""
    q = skewed(rng, nq, d, offset=0.0)
    neg = np.arange(nq) % 2 == 1
    m = int(neg.sum())
    if m:
        v = np.zeros((m, d), np.float32)
        v[:, 0] = -1.0
        v += 0.02 * rng.standard_normal((m, d)).astype(np.float32)
        q[neg] = v * np.exp(rng.uniform(-3, 3, (m, 1))).astype(np.float32)
    return q, neg


# ---------------------------------------------------------------- preparation
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prepare_stores_rows_as_given(va, oracle, dtype):
    rng = np.random.default_rng(31)
    raw = skewed(rng, 1000, 100)
    raw[5] = 0.0
    raw[6] = 1e-30
    raw[7] = -3.0e20
    with va.Index(100, dtype, "ip") as ix:
        ix.add(raw)
        got = ix.get_rows(0, 1000)
    want = oracle.prepare(raw, DT[dtype], METRIC_L2)
    assert np.array_equal(bits(got), bits(want))
    if dtype == "f32":
        assert np.array_equal(bits(got), bits(raw))


# ---------------------------------------------------------------- every path x dtype, norm-skewed data
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nq,path", [(1, 0), (1, 1), (3, 1), (4, 1), (5, 3)])
def test_stream_and_exact_paths(va, oracle, dtype, nq, path):
    rng = np.random.default_rng(100 + nq + path)
    raw = skewed(rng, 20000, 96)
    rq, neg = skewed_queries(rng, nq, 96)
    ids, sc, st = run_case(va, oracle, raw, rq, 10, dtype, path)
    assert st["path"] == (1 if path == 0 else path)
    if neg.any():
        assert (sc[neg] < 0).all()          # the best scores of those queries are all negative


@pytest.mark.parametrize("nq", [5, 40, 64])
def test_skinny_mfma_bf16(va, oracle, nq):
    rng = np.random.default_rng(200 + nq)
    raw = skewed(rng, 20000, 96)
    rq, neg = skewed_queries(rng, nq, 96)
    ids, sc, st = run_case(va, oracle, raw, rq, 10, "bf16", 2)
    assert st["path"] == 2 and (sc[neg] < 0).all()


def test_four_wave_mfma_bf16_multi_stage(va, oracle):
    """>= 65 queries take the 4-wave kernel; 300k rows make a staged search (sample pass + filtered stages)."""
    rng = np.random.default_rng(301)
    raw = skewed(rng, 300_000, 64)
    rq, neg = skewed_queries(rng, 300, 64)
    ids, sc, st = run_case(va, oracle, raw, rq, 10, "bf16", 2)
    assert st["path"] == 2 and st["scan_launches"] >= 3, st
    assert (sc[neg] < 0).all()


@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("nq", [20, 40, 300])
def test_fp32_matrix_core_and_split_passes(va, oracle, split, nq):
    rng = np.random.default_rng(400 + nq)
    raw = skewed(rng, 30000, 96)
    rq, neg = skewed_queries(rng, nq, 96)
    ids, sc, st = run_case(va, oracle, raw, rq, 10, "f32", 2, split=split)
    assert st["path"] == 2 and (sc[neg] < 0).all()


# ---------------------------------------------------------------- duplicates, near-ties, k at the edges
def test_duplicates_are_resolved_by_the_band_pass(va, oracle):
    raw = oracle.synth_rows(1, 0, 4000, 256, threads=THREADS)
    dup = np.concatenate([raw, np.repeat(raw[:8], 40, axis=0)]) * np.float32(3.5)
    q = dup[:8] * np.float32(0.25)
    ids, sc, st = run_case(va, oracle, dup, q, 10, "bf16", 2)
    assert st["fallback_queries"] > 0 and st["band_queries"] > 0, st


def test_duplicates_on_the_stream_path_take_the_exact_path(va, oracle):
    rng = np.random.default_rng(78)
    base = skewed(rng, 3000, 64, offset=0.0, lo=-0.5, hi=0.5)
    dup = np.repeat(rng.standard_normal((1, 64)).astype(np.float32) * 2, 200, axis=0)
    raw = np.concatenate([base[:1500], dup, base[1500:]])
    rq = dup[:3] + 0.01 * rng.standard_normal((3, 64)).astype(np.float32)
    for dtype in ("f32", "bf16"):
        ids, sc, st = run_case(va, oracle, raw, rq, 20, dtype, 1)
        assert st["fallback_queries"] == 3 and st["band_queries"] == 0, st


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("path", [0, 2, 3])
def test_k_one_all_beyond_and_max(va, oracle, dtype, path):
    import vrod_amd
    rng = np.random.default_rng(500 + path)
    raw = skewed(rng, 3000, 40)
    rq, _ = skewed_queries(rng, 6, 40)
    n = raw.shape[0]
    for k in (1, n, n + 77):
        ids, sc, st = run_case(va, oracle, raw, rq, k, dtype, path)
        if k > n:
            assert (ids[:, n:] == vrod_amd.ID_NONE).all() and np.isnan(sc[:, n:]).all()
    raw = skewed(rng, 5000, 40)
    run_case(va, oracle, raw, rq, vrod_amd.MAX_K, dtype, path)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("path", [0, 1, 2, 3])
def test_zero_query(va, oracle, dtype, path):
    rng = np.random.default_rng(600)
    raw = skewed(rng, 5000, 72)
    rq = np.zeros((2, 72), np.float32)
    rq[1] = skewed(rng, 1, 72)[0]
    ids, sc, st = run_case(va, oracle, raw, rq, 10, dtype, path)
    assert (bits(sc[0]) == 0).all() and ids[0].tolist() == list(range(10))


# ---------------------------------------------------------------- overflow: +inf, -inf and NaN scores
def overflow_case(rng, n=2000, d=8):
    raw = rng.standard_normal((n, d)).astype(np.float32)
    pos = rng.choice(n, 150, replace=False)
    up, down, both = pos[:50], pos[50:100], pos[100:]
    raw[up, 0] = 1e20                                   # q0 . x = +inf
    raw[down, 0] = -1e20                                # -inf
    raw[both, 0], raw[both, 1] = 1e20, -1e20            # +inf + -inf = NaN
    q0 = np.ones(d, np.float32)
    q0[:2] = 1e20
    rq = np.stack([q0, np.zeros(d, np.float32), rng.standard_normal(d).astype(np.float32), -q0,
                   q0 * np.float32(0.5), rng.standard_normal(d).astype(np.float32) * 3]).astype(np.float32)
    return raw, rq, np.sort(both)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nq", [4, 6])
def test_overflowing_dot_products(va, oracle, dtype, nq):
    """Canonical scores include +inf, -inf and NaN.  The bound is not finite (a squared row norm overflows): the
    certificate refuses every query and the exact path answers -- NaN rows last, by id, with their ids."""
    rng = np.random.default_rng(700)
    raw, rq, nan_rows = overflow_case(rng)
    rq = rq[:nq]
    n = raw.shape[0]
    oi, osc = oracle_ip(oracle, raw, rq, n, dtype)
    assert np.isposinf(osc[0]).any() and np.isneginf(osc[0]).any() and np.isnan(osc[0]).sum() == len(nan_rows)
    for path in (0, 3):
        ids, sc, st = run_case(va, oracle, raw, rq, n, dtype, path, expect=(oi, osc))
        if path == 0:
            assert st["fallback_queries"] == nq, st
        assert ids[0, -len(nan_rows):].tolist() == nan_rows.tolist()
        assert np.isnan(sc[0, -len(nan_rows):]).all() and not np.isnan(sc[0, :-len(nan_rows)]).any()
        assert (bits(sc[1]) == 0).all() and ids[1].tolist() == list(range(n))


# ---------------------------------------------------------------- pipelined, multi-device and merge forms
@pytest.mark.parametrize("dtype,path,nq", [("bf16", 2, 40), ("bf16", 2, 300), ("f32", 1, 3), ("f32", 2, 40)])
def test_pipelined_equals_search(va, oracle, dtype, path, nq):
    import torch
    rng = np.random.default_rng(800 + nq)
    raw = skewed(rng, 20000, 96)
    batches = [skewed_queries(rng, nq, 96)[0] for _ in range(4)]
    dev = torch.device("cuda", 0)
    k = 10
    with va.Index(96, dtype, "ip") as ix:
        ix.add(raw)
        ix.set_path(path)
        seq = [ix.search(b, k) for b in batches]
        dq = [torch.from_numpy(b).to(dev) for b in batches]
        outs = [(torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
                for _ in batches]
        ix.search_begin_device(dq[0], k, *outs[0])
        for s in range(len(batches)):
            if s + 1 < len(batches):
                ix.search_begin_device(dq[s + 1], k, *outs[s + 1])
                assert ix.pending == 2
            ix.search_end()
            check_bound(ix.last_stats(), f"pipelined {dtype}/{path}")
        assert ix.pending == 0
    for s, b in enumerate(batches):
        oi, osc = oracle_ip(oracle, raw, b, k, dtype)
        assert_same(*seq[s], oi, osc, f"search {s}")
        assert_same(outs[s][0].cpu().numpy().view(np.uint64), outs[s][1].cpu().numpy(), oi, osc, f"pipelined {s}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_multi_device_handle_equals_single(va, oracle, dtype):
    rng = np.random.default_rng(900)
    raw = skewed(rng, 70000, 32)              # 70000 rows: both shards hold rows
    for nq in (5, 40):
        rq, _ = skewed_queries(rng, nq, 32)
        oi, osc = oracle_ip(oracle, raw, rq, 7, dtype)
        with va.Index(32, dtype, "ip") as one:
            one.add(raw)
            si, ss = one.search(rq, 7)
        with va.Index(32, dtype, "ip", devices=[0, 0]) as two:
            two.add(raw)
            mi, ms = two.search(rq, 7)
        assert_same(si, ss, oi, osc, f"single {dtype}/{nq}")
        assert_same(mi, ms, oi, osc, f"two shards {dtype}/{nq}")


def test_merge_topk_device_and_packed_with_metric_2(va, oracle):
    """Per-shard IP lists that hold +inf, -inf and NaN scores merge like the oracle's merge in the dot order."""
    import torch
    from vrod_amd.shard import alloc_packed
    rng = np.random.default_rng(1000)
    raw, rq, _ = overflow_case(rng, n=600)
    raw[rng.choice(600, 150, replace=False), :2] = [1e20, -1e20]      # plenty of NaN rows in every shard
    nq, k, cuts = 4, 180, [0, 200, 400, 600]
    li, ls = [], []
    for g in range(3):
        i, s = oracle_ip(oracle, raw[cuts[g]:cuts[g + 1]], rq[:nq], k, "f32", id_offset=cuts[g])
        li.append(i)
        ls.append(s)
    li, ls = np.stack(li), np.stack(ls)
    assert np.isnan(ls).any() and np.isinf(ls).any()
    oi, osc = oracle.merge_topk(li, ls, METRIC_COSINE)
    dev = torch.device("cuda", 0)
    ti = torch.from_numpy(li.view(np.int64)).to(dev)
    ts = torch.from_numpy(ls).to(dev)
    for name in ("ip", 2):
        mi, ms = va.merge_topk_device(0, name, ti, ts)
        assert_same(mi.cpu().numpy().view(np.uint64), ms.cpu().numpy(), oi, osc, f"merge {name}")
    blocks = []
    for g in range(3):
        packed, pi, ps = alloc_packed(nq, k, dev)
        pi.copy_(ti[g])
        ps.copy_(ts[g])
        blocks.append(packed)
    gathered = torch.cat(blocks)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    va.merge_topk_packed_device(0, "ip", gathered, 3, nq, k, out_i, out_s)
    assert_same(out_i.cpu().numpy().view(np.uint64), out_s.cpu().numpy(), oi, osc, "packed merge")


# ---------------------------------------------------------------- host CLI end to end
def test_cli_ip_collection_end_to_end(va, oracle, tmp_path):
    if not os.path.exists(VROD):
        subprocess.run(["make", "-C", os.path.join(ROOT, "vrod_amd", "host")], check=True)

    def run(*args):
        return subprocess.run([VROD, *args], capture_output=True, text=True)

    rng = np.random.default_rng(1100)
    n, dim, nq, k = 3000, 48, 5, 7
    raw = skewed(rng, n, dim)
    rq, _ = skewed_queries(rng, nq, dim)
    emb = tmp_path / "emb.txt"
    with open(emb, "w") as f:
        for i in range(n):
            f.write(",".join(repr(float(v)) for v in raw[i]) + f";word{i}\n")
    assert run("-i", str(tmp_path), "-n", "d").returncode == 0
    db = str(tmp_path / "d")
    assert run("-d", db, "-e", "CREATE", "-a", "c metric=ip dtype=f32").returncode == 0
    r = run("-d", db, "-c", "c", "-e", "BULKINSERT", "-a", str(emb))
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "d" / "c" / "vr_config").read().split() == [f"dim={dim}", "metric=ip", "dtype=f32", f"count={n}"]
    qarg = f"k={k};" + ";".join(",".join(repr(float(v)) for v in rq[i]) for i in range(nq))
    outs = []
    for _ in range(2):                           # every run is a fresh process: load, lazy upload, search
        r = run("-d", db, "-c", "c", "-e", "SEARCHSIMILAR", "-a", qarg)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    rows = [l.split("\t") for l in outs[0].strip().split("\n")]
    assert len(rows) == nq * k
    ids = np.array([int(x[2]) for x in rows], dtype=np.uint64).reshape(nq, k)
    sc = np.array([float(x[3]) for x in rows], dtype=np.float32).reshape(nq, k)
    oi, osc = oracle_ip(oracle, raw, rq, k, "f32")
    assert_same(ids, sc, oi, osc, "cli")
    assert rows[0][4] == f"word{int(oi[0, 0])}"
    r = run("-d", db, "-e", "LISTCOLLECTIONS")
    assert r.returncode == 0 and r.stdout.split() == ["c"]
    assert "metric=ip" in open(tmp_path / "d" / "c" / "vr_config").read()
