"""The shape arithmetic of tests/test_gpu_w4_forms.py, on the CPU: every shape that file runs was chosen for a condition
-- a loop form, a launch count, a tile range of one, two, four or five tiles, a sample form, a pacing point, a route --
and a change to the planner that empties one of these cases fails here, not quietly on the GPU.

The conditions are restated from the library the way the GPU tests restate them (test_gpu_steal.stage_plan, which
tests/test_search_plan.py checks against search_plan.h; stage_strip_lens and sample_is_grouped of
test_gpu_w4_tile_loop.py; support.takes_segments).  They are asked for a device of 256 CUs (the MI355X) and of 304.
Two of them hold on 256 CUs only, by arithmetic: 170 000 rows over 152 strips give ranges of 3 and 4 tiles, not 4 and 5,
and 8448 queries fit the 38 work-group slots of one launch.  The GPU tests assert both on the device they run on; here the
304-CU values are stated as they are, and the pacing point is shown to fall inside a 3-tile range as well.
"""
import numpy as np
import pytest

from support import PATH_AUTO, PATH_MFMA, takes_segments
from test_gpu_steal import stage_plan
from test_gpu_w4_forms import (ALLOWED_SHARE, B_DIMS, B_MANY_NQ, B_MANY_ROWS, B_N, C_DIMS, C_N, GROWN_ROWS, K, LIST_CAP, NQ, WIDTHS, allow_list,
                               deleted_stretch, k_tiles, plan_metric, scan_launches, tloop_pace_tiles)
from test_gpu_w4_tile_loop import sample_is_grouped, stage_strip_lens, takes_tile_loop

CUS = (256, 304)
ORACLE_CAP = 2.5e9                   # n * nq * dim of one oracle call (tests/test_gpu_random.py)


def test_the_widths_take_the_loop_form_the_table_says():
    want = {256: (4, True), 384: (6, True), 768: (12, True), 200: (4, True), 192: (3, False), 320: (5, False)}
    assert {d: w[:2] for d, w in WIDTHS.items()} == want
    for dim, (kt, tile_loop) in want.items():
        assert k_tiles(dim) == kt and takes_tile_loop(dim) == tile_loop, dim
        assert kt >= 3                                     # the flat controls too run the `tile = st_tile` arm
    assert {w[2] for d, w in WIDTHS.items() if w[1]} == {"cosine", "l2", "ip"}             # each metric meets the tile loop
    assert [d for d, w in WIDTHS.items() if w[3]] == [384]
    for dim in B_DIMS + C_DIMS + (256,):
        assert takes_tile_loop(dim)


@pytest.mark.parametrize("num_cus", CUS)
def test_the_handle_scripts_run_one_launch_and_then_a_sample_and_two_filtered_launches(num_cus):
    """A corpus that fits one hit list is one filtered launch; the last case's handle, grown to GROWN_ROWS, is staged."""
    assert GROWN_ROWS > LIST_CAP and GROWN_ROWS % 256 != 0 and GROWN_ROWS * NQ * max(WIDTHS) <= ORACLE_CAP
    for dim, (_, _, metric, _, n) in WIDTHS.items():
        assert n % 256 != 0 and n == (2003 if dim == 768 else 5003)
        assert n <= LIST_CAP and scan_launches(n, NQ, K, metric, num_cus) == 1
        for nq in (NQ, 257):
            assert nq > 64 and (nq + 255) // 256 == 2
        for k in (K, 100):
            kp, sample, bounds = stage_plan(GROWN_ROWS, NQ, k, plan_metric(metric), num_cus)
            assert len(bounds) == 2 and bounds[-1] == GROWN_ROWS and sample < bounds[0] < GROWN_ROWS, (dim, bounds)
            assert scan_launches(GROWN_ROWS, NQ, k, metric, num_cus) == 3
            assert not sample_is_grouped(sample, kp)                                        # the every-score sample
        _, _, lens = stage_strip_lens(GROWN_ROWS, NQ, K, plan_metric(metric), num_cus)
        assert all(set(stage) <= {0, 1} and 1 in stage for stage in lens), (dim, lens)      # ranges of one tile, and idle strips


@pytest.mark.parametrize("num_cus", CUS)
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_60000_rows_end_on_ranges_of_one_and_of_two_tiles(num_cus, metric):
    _, _, lens = stage_strip_lens(B_N, NQ, K, metric, num_cus)
    assert len(lens) == 2
    assert 1 in lens[-1] and 2 in lens[-1] and max(lens[-1]) == 2, lens[-1]
    assert B_N % 256 != 0


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_170000_rows_end_on_ranges_of_four_and_five_tiles(metric):
    sample, kp, lens = stage_strip_lens(C_N, NQ, K, metric, 256)
    assert set(lens[-1]) == {4, 5} and sample_is_grouped(sample, kp)                        # the group-best sample form
    sample, kp, lens = stage_strip_lens(C_N, NQ, K, metric, 304)
    assert set(lens[-1]) == {3, 4} and sample_is_grouped(sample, kp)                        # (152 strips: a tile shorter)


def test_both_sample_forms_occur():
    for num_cus in CUS:
        forms = set()
        for n, k in ((C_N, K), (B_N, K), (B_N, 100), (GROWN_ROWS, K), (GROWN_ROWS, 100)):
            kp, sample, _ = stage_plan(n, NQ, k, "cosine", num_cus)
            forms.add(sample_is_grouped(sample, kp))
        assert forms == {True, False}


def test_33_query_blocks_need_two_launches_on_256_cus():
    assert B_MANY_NQ == 33 * 256 and B_MANY_ROWS % 256 != 0
    slots = lambda num_cus: max(8, num_cus // 8 * 8) // 8                                   # launch_scan_mfma: a query block per work-group slot
    assert slots(256) == 32 and 256 * slots(256) < B_MANY_NQ                                # launches of 32 blocks and of 1: qb_base = 32
    assert slots(304) == 38 and 256 * slots(304) >= B_MANY_NQ                               # (one launch there)
    assert B_MANY_ROWS <= LIST_CAP and scan_launches(B_MANY_ROWS, B_MANY_NQ, K, "cosine", 256) == 1   # one stage: two kernel launches in all


@pytest.mark.parametrize("dim", C_DIMS)
def test_the_pacing_countdown_fires_inside_a_short_range_at_8_k_tiles_only(dim):
    kt = k_tiles(dim)
    assert kt in (4, 6)
    for ntiles in (3, 4, 5):                               # the ranges at 170 000 rows, 256 and 304 CUs
        fired = tloop_pace_tiles(kt, 8, ntiles)
        assert fired and fired[0] == 3, (dim, ntiles, fired)                                # first in front of the range's third tile
        assert tloop_pace_tiles(kt, 192, ntiles) == [] and tloop_pace_tiles(kt, 0, ntiles) == []
    assert tloop_pace_tiles(4, 8, 9) == [3, 5, 7, 9]       # every two tiles after that
    assert tloop_pace_tiles(6, 8, 9) == [3, 4, 5, 7, 8, 9]  # three tiles in four (6 K-tiles a tile, 8 a point)
    # the default never fires on a range without a stolen tail (fewer than 48 tiles): 192 K-tiles are 48 and 32 tiles
    assert tloop_pace_tiles(4, 192, 48) == [] and tloop_pace_tiles(4, 192, 49) == [49]
    assert tloop_pace_tiles(6, 192, 33) == [33]
    assert NQ > 256                                        # two query blocks: a.nqb > 1, so the launcher paces at all


def test_the_allow_list_of_the_handle_scripts_takes_the_dense_route():
    for dim, (_, _, _, _, n) in WIDTHS.items():
        allow = allow_list(dim, n)
        assert abs(allow.mean() - ALLOWED_SHARE) < 0.03
        gone = np.zeros(n, bool)
        gone[deleted_stretch(n)] = True
        hi = int((allow & ~gone).sum())                    # eligible rows before the 100 queries' best rows go too
        for m in (hi - 100, hi):
            assert 0.4 * n < m < 0.65 * n
            assert not takes_segments(PATH_AUTO, "bf16", n, m, NQ, dim) and not takes_segments(PATH_MFMA, "bf16", n, m, NQ, dim), (dim, m)
