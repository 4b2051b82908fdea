"""GPU tests of the host forms of add, update and upsert at the boundaries of the kernel that prepares their rows.

vrod_index_add, _add_synthetic, _update and _upsert stage their fp32 rows on the device at a stride of dim and prepare
them with ingest_rows_kernel.  Which of its variants a host call gets depends on three things:
  dim % 4         16-byte loads only where dim * 4 is a multiple of 16 (the staging buffer itself is aligned)
  dim <= 4096     four rows per work-group, a wave each; beyond that one row per work-group
  the metric      cosine normalises through LDS, l2 and ip stream
Truth is the CPU oracle's prepare, bit for bit, read back through get_rows.  Row counts: 1, 5 (a ragged last group of
four) and 70 (more than one work-group), and 3 at the widest rows as well."""
import numpy as np
import pytest

from support import DT, O, THREADS, bits, prep_of, special_rows, va  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID_VALUE = 2
HANDLES = (("bf16", "cosine"), ("f32", "l2"))
DIMS = (1, 3, 4, 5, 63, 64, 65, 4096, 4097, 4099, 32768)


def rows_for(n, dim, seed):
    """n of special_rows' rows, the special ones among them at every n: 70 holds them all, 5 the two scaled rows, the
    zero row, the -0.0 row and the subnormals, 3 a scaled row, the zero row and the -0.0 row, 1 the -0.0 row."""
    x = special_rows(max(n, 16), dim, seed, "f32")
    first = {70: 0, 5: 1, 3: 2, 1: 4}[n]
    return np.ascontiguousarray(x[first: first + n])


def prepared(O, rows, dtype, metric):
    return bits(O.prepare(rows, DT[dtype], prep_of(metric), threads=THREADS))


@pytest.mark.parametrize("dim", DIMS)
def test_add_then_update_at_this_width(va, O, dim):
    for dtype, metric in HANDLES:
        for n in (1, 5, 70) + ((3,) if dim == 32768 else ()):
            what = f"dim {dim} n {n} {dtype}/{metric}"
            now = rows_for(n, dim, dim * 5 + n)
            with va.Index(dim, dtype, metric) as ix:
                ix.add(now)
                assert ix.count == n
                assert np.array_equal(bits(ix.get_rows(0, n)), prepared(O, now, dtype, metric)), f"{what}: add"
                upd = rows_for(3, dim, dim * 5 + n + 1)[:2]    # a scaled row, then the zero row
                ix.update([n - 1, n - 1], upd)                 # one id named twice: the last vector wins
                now[n - 1] = upd[1]
                assert ix.count == n
                assert np.array_equal(bits(ix.get_rows(0, n)), prepared(O, now, dtype, metric)), f"{what}: update"


@pytest.mark.parametrize("dtype,metric", HANDLES)
def test_a_nan_in_the_ragged_group_refuses_the_add(va, O, dtype, metric):
    """The last row of five at dim 4097: the one-row-per-group variant, elements read one by one."""
    dim = 4097
    base = rows_for(70, dim, 7)
    q = rows_for(3, dim, 8)
    with va.Index(dim, dtype, metric) as ix:
        ix.add(base)
        ix.search(q, 5)
        eps = bits(ix.last_stats()["eps_bound"]).tolist()
        bad = rows_for(5, dim, 9)
        bad[4, dim - 1] = np.nan
        with pytest.raises(va.VrodError) as e:
            ix.add(bad)
        assert e.value.code == INVALID_VALUE
        assert ix.count == 70
        assert np.array_equal(bits(ix.get_rows(0, 70)), prepared(O, base, dtype, metric))
        ix.search(q, 5)
        assert bits(ix.last_stats()["eps_bound"]).tolist() == eps
        ix.add(bad[:4])                                        # the rows before it are fine, and the flag was cleared
        assert np.array_equal(bits(ix.get_rows(70, 4)), prepared(O, bad[:4], dtype, metric))


@pytest.mark.parametrize("dtype,metric", HANDLES)
def test_add_synthetic(va, O, dtype, metric):
    dim, n, seed, first = 65, 70, 5, 1000
    with va.Index(dim, dtype, metric) as ix:
        ix.add_synthetic(seed, first, n)
        assert ix.count == n
        assert np.array_equal(bits(ix.get_rows(0, n)), prepared(O, O.synth_rows(seed, first, n, dim), dtype, metric))


@pytest.mark.parametrize("dtype,metric", HANDLES)
def test_upsert_with_held_and_new_keys_interleaved(va, O, dtype, metric):
    """The held rows and the new rows are each a list of the call's rows, gathered for their upload."""
    dim, n0, n = 65, 20, 9
    base = rows_for(70, dim, 11)[:n0]
    keys0 = np.arange(n0, dtype=np.uint64) * np.uint64(7919) + np.uint64(13)
    rows = rows_for(70, dim, 12)[:n]
    keys = np.empty(n, np.uint64)
    keys[0::2] = np.arange(5, dtype=np.uint64) + np.uint64(1 << 50)    # new, in the order of the call
    keys[1::2] = keys0[[17, 2, 11, 5]]                                 # held
    with va.Index(dim, dtype, metric) as ix:
        ix.add(base)
        ix.set_keys(0, keys0)
        ids = ix.upsert(keys, rows)
        assert ids.tolist() == [20, 17, 21, 2, 22, 11, 23, 5, 24] and ix.count == n0 + 5
        now = np.concatenate([base, np.zeros((5, dim), np.float32)])
        now[ids.astype(np.int64)] = rows
        got, want = bits(ix.get_rows(0, ix.count)), prepared(O, now, dtype, metric)
        for r in range(ix.count):
            assert np.array_equal(got[r], want[r]), f"row {r}"
