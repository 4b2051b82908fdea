"""Work stealing of the 4-wave scan (kernels_mfma_w4.hip): the last 1/16 of every strip's tiles is handed out in chunks
that any work-group of the same query block may claim.  Needs strips of at least 48 tiles and K extents of at least three
K-tiles, i.e. a corpus the small parity cases never reach: 1.5M x 192 bf16, batch 1024 -- the last filtered stage walks
~73 tiles per strip.  Every (chunk, query block) pair must be scanned exactly once whoever claims it: ids and score bits
of the whole batch = the oracle's; and the same with stealing switched off (VROD_DEBUG_W4_STEAL=0, own process).
Parity unpinned by the reference (vRod holds no scan): the oracle is build-authored.

An ODD tail (the shard sizes of the multi-GPU plan: 1.25M rows -> 3 tiles, 2.5M -> 7, 5M -> 11) is cut into chunks of 2
with the odd tile folded into the last one (vrod_amd/csrc/w4_steal.h): 1.3M rows give strips of 54-55 tiles, tail 3 (one
chunk of 3), 1.85M give 87-88, tail 5 (2 + 3).  The stage plan and launch geometry are restated below, and the tests
assert that the restatement still matches the library (its launch count) and still gives the odd tail they are for."""
import os
import subprocess
import sys

import numpy as np
import pytest

from support import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stage_plan(n, nq, k, metric, num_cus):
    """Restated from the library for a bf16 batch on a fresh handle (candidate margin x1): k' (search_plan.h
    choose_kp), the sample rows S and the stage bounds (search_plan.h plan_stages).  tests/test_search_plan.py checks
    this restatement against the header on the CPU.  Returns (k', S, bounds)."""
    tile, cap = 256, 8192
    kp = min(n, cap // 2, k + max(8 if metric == "cosine" else 16, k // 8))
    nqb = (nq + 255) // 256
    g = max(2, min(5, cap // (3 * kp)))
    max_sample = max(1, num_cus // nqb) * tile
    S = min(n // (g * g), max_sample)
    S = max(S, min(n, max(4 * kp, tile)))
    S = min((S + tile - 1) // tile * tile, n)
    bounds, b = [], S * g
    while b < n:
        if n - b < b / 2:
            break
        bounds.append(b // tile * tile)
        b *= g
    bounds.append(n)
    return kp, S, bounds


def last_stage_plan(n, nq, k, metric, num_cus):
    """stage_plan, the launch geometry of launch_scan_mfma for the 4-wave kernel, and w4_tail_tiles (w4_steal.h,
    default VROD_W4_STEAL_DIV 16 / VROD_W4_STEAL_CHUNK 2).  Returns (scan launches, the set of tails of the last
    filtered launch's strips, the strip lengths)."""
    tile = 256
    _, _, bounds = stage_plan(n, nq, k, metric, num_cus)
    nqb = (nq + 255) // 256
    grid = max(8, num_cus // 8 * 8)
    nstrips = 8 * ((grid // 8) // nqb)
    first = bounds[-2] // tile
    ntiles = (n + tile - 1) // tile - first
    lens = {ntiles * (s + 1) // nstrips - ntiles * s // nstrips for s in range(nstrips)}
    tail = lambda t: 0 if t < 48 else min(t // 16, 64)
    return 1 + len(bounds), {tail(t) for t in lens}, lens


def _oracle_parity(oracle, n, metric, want_tail=None):
    import torch
    assert torch.cuda.is_available()
    import vrod_amd as va
    dim, nq, k = 192, 1024, 10
    launches, tails, lens = last_stage_plan(n, nq, k, metric, torch.cuda.get_device_properties(0).multi_processor_count)
    if want_tail is not None:
        assert tails == {want_tail} and want_tail % 2 == 1, (tails, lens)
    raw = oracle.synth_rows(91, 0, n, dim, threads=16)
    rq = oracle.synth_rows(92, 0, nq, dim, threads=16)
    oi, osc = oracle.search(raw, rq, k, 1, {"cosine": 0, "l2": 1}[metric], threads=16)
    with va.Index(dim, "bf16", metric) as ix:
        ix.add(raw)
        ix.set_path(va.PATH_MFMA)
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
    assert st["path"] == va.PATH_MFMA and st["scan_launches"] >= 3, st
    if want_tail is not None:
        assert st["scan_launches"] == launches, (st, launches)   # the restated plan is the library's
    assert np.array_equal(ids, oi), np.argwhere(ids != oi)[:5]
    assert np.array_equal(bits(sc), bits(osc))


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_batch_over_long_strips_equals_the_oracle(oracle, metric):
    _oracle_parity(oracle, 1_500_000, metric)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("n,tail", [(1_300_000, 3), (1_850_000, 5)])
def test_odd_tails_equal_the_oracle(oracle, metric, n, tail):
    """Strips whose tail is odd: the last chunk holds 3 tiles (never a 1-tile range: w4_steal.h)."""
    _oracle_parity(oracle, n, metric, want_tail=tail)


def _steal_on_off(n):
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, ".")
import vrod_amd as va
ix = va.Index(192, "bf16", "cosine"); ix.add_synthetic(1, 0, int(sys.argv[2])); ix.set_path(va.PATH_MFMA)
oi = torch.empty((1024, 10), dtype=torch.int64, device="cuda"); osc = torch.empty((1024, 10), dtype=torch.float32, device="cuda")
ix.search_synthetic_device(2, 0, 1024, 10, oi, osc); torch.cuda.synchronize()
np.save(sys.argv[1], np.concatenate([oi.cpu().numpy().astype(np.int64), osc.cpu().numpy().view(np.int32).astype(np.int64)], axis=1))
'''
    outs = []
    for mode in ("1", "0"):
        path = f"/tmp/vrod_steal_{os.getpid()}_{n}_{mode}.npy"
        env = dict(os.environ, VROD_DEBUG_W4_STEAL=mode)
        r = subprocess.run([sys.executable, "-c", code, path, str(n)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(path))
        os.unlink(path)
    assert np.array_equal(outs[0], outs[1])


def test_stealing_off_gives_the_same_bits():
    _steal_on_off(1_500_000)


def test_stealing_off_gives_the_same_bits_on_an_odd_tail():
    import torch
    _, tails, lens = last_stage_plan(1_300_000, 1024, 10, "cosine", torch.cuda.get_device_properties(0).multi_processor_count)
    assert tails == {3}, (tails, lens)
    _steal_on_off(1_300_000)
