"""The tile loop of the 4-wave scan (kernels_mfma_w4.hip, TLOOP): launches whose K extent is an even number of K-tiles,
at least 4, run a loop over tiles around a fixed-trip K loop; every other K extent keeps the flat loop.  Ids and score
bits of a bf16 batch must equal the CPU oracle's under both forms, with the MFMA path forced.

Shapes.  Batch 300 = two query blocks, one of them partial.  Dim 256 (4 K-tiles: the K loop between the four special
K-tiles runs zero times), 384 (6: once), 768 (12: four times); dim 320 (5 K-tiles) and 128 (2) take the flat loop.
60 000 rows: with 128 strips per launch (256 CUs, two query blocks) the last filtered stage spreads 185 tiles over the
strips, so a work-group's static range is exactly one tile or exactly two, and the corpus ends on a partial tile (96
rows) -- the three endings of the tile loop; the plan is restated from the library the way tests/test_gpu_steal.py does
it, and the tests assert that those cases still occur.  Sample forms: 170 000 rows at k = 10 take the group-best sample
(DENSE 2), k = 100 the every-score sample (DENSE 1) -- the condition of vrod_index.hip restated and asserted.

Work stealing under the tile loop: tests/test_gpu_steal.py runs at dim 192 (3 K-tiles, the flat loop); its two shapes are
repeated here at dim 256 -- 1.5M rows (even tails) and 1.3M rows (tail 3) -- against the oracle, and once each with
stealing switched off (VROD_DEBUG_W4_STEAL=0, own process): the same bits.
Parity unpinned by the reference (vRod holds no scan): the oracle is build-authored."""
import os
import subprocess
import sys

import numpy as np
import pytest

from support import bits, row_bytes
from test_gpu_steal import last_stage_plan, stage_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = 300


def takes_tile_loop(dim):
    """launch_mfma_w4, restated: bf16 rows whose K extent is an even number of 128-byte K-tiles, at least 4."""
    kt = row_bytes("bf16", dim) // 128
    return kt >= 4 and kt % 2 == 0


def stage_strip_lens(n, nq, k, metric, num_cus):
    """Per scan launch of a bf16 batch on a fresh handle, the multiset of strip lengths in tiles (launch_scan_mfma's
    geometry for the 4-wave kernel): (sample rows S, k', [lengths of filtered stage 0, 1, ...])."""
    tile = 256
    kp, S, bounds = stage_plan(n, nq, k, metric, num_cus)
    nqb = (nq + 255) // 256
    grid = max(8, num_cus // 8 * 8)
    nstrips = 8 * ((grid // 8) // nqb)
    out, lo = [], 0
    for b in bounds:
        first = lo // tile
        ntiles = (b + tile - 1) // tile - first
        out.append([ntiles * (s + 1) // nstrips - ntiles * s // nstrips for s in range(nstrips)])
        lo = b
    return S, kp, out


def sample_is_grouped(S, kp):
    """vrod_index.hip: the sample pass writes group bests (groups of 32 rows) while the groups outnumber j by 8x and the
    sample is whole tiles; else every score."""
    return S % 256 == 0 and min(kp, S) * 8 <= S // 32


def _parity(oracle, n, dim, metric, k):
    import vrod_amd as va
    raw = oracle.synth_rows(71, 0, n, dim, threads=16)
    rq = oracle.synth_rows(72, 0, NQ, dim, threads=16)
    oi, osc = oracle.search(raw, rq, k, 1, {"cosine": 0, "l2": 1}[metric], threads=16)
    with va.Index(dim, "bf16", metric) as ix:
        ix.add(raw)
        ix.set_path(va.PATH_MFMA)
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
    assert st["path"] == va.PATH_MFMA, st
    assert np.array_equal(ids, oi), (dim, metric, np.argwhere(ids != oi)[:5])
    assert np.array_equal(bits(sc), bits(osc)), (dim, metric)
    return st


def _cus():
    import torch
    assert torch.cuda.is_available()
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("dim,tile_loop", [(256, True), (384, True), (768, True), (320, False), (128, False)])
def test_ranges_of_one_tile_two_tiles_and_a_partial_last_tile(oracle, metric, dim, tile_loop):
    n, k = 60_000, 10
    assert takes_tile_loop(dim) == tile_loop
    S, kp, lens = stage_strip_lens(n, NQ, k, metric, _cus())
    assert 1 in lens[-1] and 2 in lens[-1] and max(lens[-1]) == 2, lens[-1]   # static ranges of exactly one and exactly two tiles
    assert n % 256 != 0                                                       # ... and one that ends on a partial tile
    st = _parity(oracle, n, dim, metric, k)
    assert st["scan_launches"] == 1 + len(lens), (st, len(lens))              # the restated plan is the library's


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_group_best_sample_form(oracle, metric):
    """DENSE 2 under the tile loop (dim 256), and ranges of 4 and 5 tiles behind it: tile after tile inside one range."""
    n, k = 170_000, 10
    S, kp, lens = stage_strip_lens(n, NQ, k, metric, _cus())
    assert sample_is_grouped(S, kp), (S, kp)
    assert set(lens[-1]) == {4, 5}, set(lens[-1])
    _parity(oracle, n, 256, metric, k)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_every_score_sample_form(oracle, metric):
    """DENSE 1 under the tile loop (dim 384): k = 100 asks for more sample ranks than a group-best sample holds."""
    n, k = 60_000, 100
    S, kp, _ = stage_strip_lens(n, NQ, k, metric, _cus())
    assert not sample_is_grouped(S, kp), (S, kp)
    _parity(oracle, n, 384, metric, k)


# ---------------------------------------------------------------- work stealing under the tile loop (dim 256)
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("n,odd_tail", [(1_500_000, None), (1_300_000, 3)])
def test_stealing_at_dim_256_equals_the_oracle(oracle, metric, n, odd_tail):
    import vrod_amd as va
    dim, nq, k = 256, 1024, 10
    assert takes_tile_loop(dim)
    launches, tails, lens = last_stage_plan(n, nq, k, metric, _cus())
    assert min(lens) >= 48, lens                       # long strips: every one has a tail to hand out
    if odd_tail is None:
        assert all(t > 0 and t % 2 == 0 for t in tails), (tails, lens)
    else:
        assert tails == {odd_tail}, (tails, lens)
    raw = oracle.synth_rows(91, 0, n, dim, threads=16)
    rq = oracle.synth_rows(92, 0, nq, dim, threads=16)
    oi, osc = oracle.search(raw, rq, k, 1, {"cosine": 0, "l2": 1}[metric], threads=16)
    with va.Index(dim, "bf16", metric) as ix:
        ix.add(raw)
        ix.set_path(va.PATH_MFMA)
        ids, sc = ix.search(rq, k)
        st = ix.last_stats()
    assert st["path"] == va.PATH_MFMA and st["scan_launches"] == launches, (st, launches)
    assert np.array_equal(ids, oi), np.argwhere(ids != oi)[:5]
    assert np.array_equal(bits(sc), bits(osc))


@pytest.mark.parametrize("n", [1_500_000, 1_300_000])
def test_stealing_off_gives_the_same_bits_at_dim_256(n):
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, ".")
import vrod_amd as va
ix = va.Index(256, "bf16", "cosine"); ix.add_synthetic(1, 0, int(sys.argv[2])); ix.set_path(va.PATH_MFMA)
oi = torch.empty((1024, 10), dtype=torch.int64, device="cuda"); osc = torch.empty((1024, 10), dtype=torch.float32, device="cuda")
ix.search_synthetic_device(2, 0, 1024, 10, oi, osc); torch.cuda.synchronize()
np.save(sys.argv[1], np.concatenate([oi.cpu().numpy().astype(np.int64), osc.cpu().numpy().view(np.int32).astype(np.int64)], axis=1))
'''
    outs = []
    for mode in ("1", "0"):
        path = f"/tmp/vrod_steal256_{os.getpid()}_{n}_{mode}.npy"
        env = dict(os.environ, VROD_DEBUG_W4_STEAL=mode)
        r = subprocess.run([sys.executable, "-c", code, path, str(n)], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(np.load(path))
        os.unlink(path)
    assert np.array_equal(outs[0], outs[1])
