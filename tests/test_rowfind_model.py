"""CPU tests of the row-lookup model (rowfind_model) on hand-written cases: the stored side is the CPU oracle's prepare() of
a few rows (what add() stores and get_rows reads back), the input side goes through the same prepare()."""
import numpy as np

import rowfind_model
from rowfind_model import ID_NONE, lookup, prepared
from support import O  # noqa: F401

NONE = int(ID_NONE)


def run(O, dtype, metric, stored_raw, inputs, deleted=(), append=False, off=0):
    stored = prepared(O, stored_raw, dtype, metric)
    out, st, app = lookup(stored, deleted, prepared(O, inputs, dtype, metric), append, off)
    return out.tolist(), st, app


def test_scaled_copy_is_found_under_cosine_only(O):
    a = np.array([[3.0, 4.0, 0.0, -12.0], [1.0, 1.0, 1.0, 1.0]], np.float32)
    inputs = np.stack([2 * a[0], a[0], 4 * a[1]])
    out, st, _ = run(O, "f32", "cosine", a, inputs)
    assert out == [0, 0, 1] and st == {"rows": 3, "found": 3, "repeats": 0, "appended": 0}
    out, st, _ = run(O, "f32", "l2", a, inputs)
    assert out == [NONE, 0, NONE] and st["found"] == 1
    out, st, _ = run(O, "f32", "ip", a, inputs)                                  # ip stores the vectors as given, as l2
    assert out == [NONE, 0, NONE]


def test_rounded_twin_is_found_on_bf16_only(O):
    base = (np.array([[1.0, -2.5, 0.375, 7.0]], np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    twin = base * np.float32(1 + 2.0 ** -12)
    assert not np.array_equal(base, twin)
    out, _, _ = run(O, "bf16", "l2", base, twin)
    assert out == [0]
    out, _, _ = run(O, "f32", "l2", base, twin)
    assert out == [NONE]


def test_sign_of_zero_and_near_misses(O):
    a = np.array([[1.0, 2.0, 0.0, -3.5, 7.0]], np.float32)
    sign, last, first, swap = a.copy(), a.copy(), a.copy(), a.copy()
    sign[0, 2] = -0.0
    last[0, -1] = np.nextafter(a[0, -1], np.float32(np.inf))
    first[0, 0] = np.nextafter(a[0, 0], np.float32(0))
    swap[0, [1, 3]] = a[0, [3, 1]]
    assert a[0, 2] == sign[0, 2] and np.signbit(sign[0, 2])                      # equal as numbers, different bits
    out, st, _ = run(O, "f32", "l2", a, np.concatenate([a, sign, last, first, swap]))
    assert out == [0, NONE, NONE, NONE, NONE] and st["found"] == 1 and st["repeats"] == 0


def test_smallest_live_id_when_the_smallest_is_deleted(O):
    a = np.array([1.0, 2.0, 3.0], np.float32)
    stored = np.stack([a, a + 1, a, a, a + 1])
    out, st, _ = run(O, "f32", "l2", stored, a[None], off=5000)
    assert out == [5000]
    out, _, _ = run(O, "f32", "l2", stored, np.stack([a, a + 1]), deleted=[0, 1], off=5000)
    assert out == [5002, 5004]
    out, st, app = run(O, "f32", "l2", stored, np.stack([a, a + 1]), deleted=[0, 2, 3])   # every copy deleted: not found
    assert out == [NONE, 1] and st["found"] == 1 and app == [0]
    out, st, app = run(O, "f32", "l2", stored, np.stack([a, a + 1]), deleted=[0, 2, 3], append=True, off=10)
    assert out == [15, 11] and st == {"rows": 2, "found": 1, "repeats": 0, "appended": 1} and app == [0]


def test_repeats_within_the_call(O):
    a = np.array([1.0, 2.0, 3.0], np.float32)
    stored = np.stack([a, a + 1])
    new1, new2 = a + 5, a + 9
    inputs = np.stack([new1, a, new2, new1, a, new2, new1])
    out, st, app = run(O, "f32", "l2", stored, inputs)
    assert out == [NONE, 0, NONE, NONE, 0, NONE, NONE] and app == [0, 2]
    assert st == {"rows": 7, "found": 2, "repeats": 3, "appended": 0}            # a found input that repeats is found again
    out, st, app = run(O, "f32", "l2", stored, inputs, append=True, off=100)
    assert out == [102, 100, 103, 102, 100, 103, 102] and app == [0, 2]
    assert st == {"rows": 7, "found": 2, "repeats": 3, "appended": 2} and st["appended"] == st["rows"] - st["found"] - st["repeats"]
    out, st, app = run(O, "f32", "cosine", stored, np.stack([new1, 4 * new1]), append=True)   # repeats are judged on prepared bits
    assert out == [2, 2] and st["repeats"] == 1 and app == [0]
    out, st, app = run(O, "f32", "l2", np.zeros((0, 3), np.float32), np.stack([a, a, a + 1]), append=True)   # an empty handle
    assert out == [0, 0, 1] and st == {"rows": 3, "found": 0, "repeats": 1, "appended": 2}
    out, st, app = lookup(stored, (), np.zeros((0, 3), np.float32), True)
    assert out.size == 0 and st == {"rows": 0, "found": 0, "repeats": 0, "appended": 0} and app == []
    assert rowfind_model.exact(dict(st, slots=7)) == st
