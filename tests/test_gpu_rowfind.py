"""GPU tests of row lookup (vrod_index_find_rows, _add_unique and their _device forms) against rowfind_model, which matches
the CPU oracle's prepare() of the inputs with the rows get_rows reads back, by their bytes.

The shapes are those at which the duplicate passes can go wrong (test_gpu_duplicates.py; the construction is restated
here): 256 + 37 rows -- two work-groups of the hash pass, five waves of the probe pass, the last one partial -- added after
reserve(N + 300); dims 8 (one 16-byte unit per bf16 row), 33 (the word path, a half-filled last word on bf16) and 768 (the
whole wave a row); 40 rows of dim 4099 for long rows through the word path; id_offset 5000.  The lookup batch holds about
150 inputs built from the corpus's planted structure (`lookup_batch`).  Everything is exact -- ids, the four exact stats,
stored bits, score bits, snapshot bytes; of the diagnostics only batches under SMALL_BATCH and compare_misses > 0 under the
narrow hash are asserted.
"""
import ctypes as C

import numpy as np
import pytest

import rowfind_model
from rowfind_model import ID_NONE, exact
from support import O, va, assert_same, bits  # noqa: F401

pytestmark = pytest.mark.gpu

N = 256 + 37
G = 256
OFF = 5000
NONE = int(ID_NONE)
ERR_INVALID_ARG, ERR_INVALID_VALUE, ERR_UNSUPPORTED = 1, 2, 6
CASES = [(dt, me, d) for dt in ("bf16", "f32") for me in ("cosine", "l2") for d in (8, 33, 768)] + [("bf16", "ip", 33)]
LONG = [("bf16", "cosine", 4099), ("f32", "l2", 4099)]


def bf16_exact(x):
    """fp32 values whose low 16 bits are zero: bf16 stores them as they are."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def planted(dim, n=N, seed=1):
    """Random rows with the planted structure, the rows to delete, and where everything is."""
    rng = np.random.default_rng(seed * 1000 + dim)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    p = {}
    edge = min(G, n - 20)
    free = [int(r) for r in rng.permutation(n) if r not in (edge - 1, edge)]
    take = lambda m: sorted(free.pop() for _ in range(m))
    x[edge] = x[edge - 1]                                                        # a pair straddling the work-group edge
    p["edge"] = [edge - 1, edge]
    p["big"] = take(100 if n >= N else 5)                                        # a large class spread over the range
    x[p["big"]] = x[p["big"][0]]
    p["first_dead"] = take(4)                                                    # its smallest id is deleted: the next live one is the first
    x[p["first_dead"]] = x[p["first_dead"][0]]
    p["lone"] = take(3)                                                          # every copy deleted
    x[p["lone"]] = x[p["lone"][0]]
    p["z"] = take(1)                                                             # a bf16-exact row with a zero: the near-misses are built from it
    z = bf16_exact(rng.standard_normal(dim).astype(np.float32))
    z[2], z[1], z[dim - 2] = 0.0, np.float32(0.75), np.float32(-1.25)
    x[p["z"][0]] = z
    p["scaled"] = take(2)                                                        # a row and twice that row: one class under cosine
    x[p["scaled"][1]] = 2.0 * x[p["scaled"][0]]
    p["rounded"] = take(2)                                                       # two fp32 rows that round to one bf16 row
    x[p["rounded"][0]] = bf16_exact(x[p["rounded"][0]])
    x[p["rounded"][1]] = x[p["rounded"][0]] * np.float32(1 + 2.0 ** -12)
    p["solo"] = take(12)                                                         # rows without a copy that stay alive
    dead = [p["first_dead"][0]] + p["lone"]
    p["dead_solo"] = [int(r) for r in rng.choice(free, min(60, len(free) // 2), replace=False)]   # the random deletes leave the planted rows alone
    p["dead"] = np.array(sorted(dead + p["dead_solo"]), np.uint64)
    return x, p


def lookup_batch(x, p, dim, seed=7, fresh=100):
    """About 150 inputs built from the planted structure -> (inputs, where each kind sits)."""
    rng = np.random.default_rng(seed * 100 + dim)
    z = x[p["z"][0]]
    last, first, sign, swap = z.copy(), z.copy(), z.copy(), z.copy()
    last[-1] *= np.float32(1.5)                                                  # only the last element differs
    first[0] *= np.float32(1.5)                                                  # only the first
    sign[2] = np.float32(-0.0)                                                   # only the sign of a zero
    swap[[1, dim - 2]] = z[[dim - 2, 1]]                                         # two elements swapped
    new = rng.standard_normal((fresh, dim)).astype(np.float32)
    big = p["big"]
    rows, at = [], {}

    def put(name, *vs):
        at[name] = list(range(len(rows), len(rows) + len(vs)))
        rows.extend(np.asarray(v, np.float32) for v in vs)

    put("new_a", *new[:fresh // 2])
    put("big", x[big[len(big) // 2]])                                            # a copy of a row of the large class: its smallest live id
    put("first_dead", x[p["first_dead"][2]])                                     # the class's smallest id is deleted: the next live one
    put("all_dead", x[p["lone"][1]], x[p["dead_solo"][0]])                       # every copy is deleted
    put("two_x", 2.0 * x[p["solo"][0]])                                          # found under cosine only
    put("twin", z * np.float32(1 + 2.0 ** -12))                                  # found on a bf16 handle only
    put("near", last, first, sign, swap)                                         # the four near-misses
    put("z", z)
    put("solo", *x[p["solo"]])
    put("edge", x[p["edge"][1]])
    put("scaled", x[p["scaled"][1]], x[p["scaled"][0]])
    put("rounded", x[p["rounded"][1]])
    put("new_b", *new[fresh // 2:])
    put("again", new[3], x[big[-1]], 2.0 * x[p["solo"][0]], new[3], new[fresh - 1], last, x[p["lone"][1]], new[3])   # repeats inside the call
    return np.stack(rows), at


@pytest.fixture(scope="module")
def worlds():
    w = {d: planted(d) for d in (8, 33, 768)}
    w[4099] = planted(4099, n=40)
    return {d: (x, p) + lookup_batch(x, p, d) for d, (x, p) in w.items()}


def filled(va, worlds, dtype, metric, dim, off=OFF, keys=False, reserve=True, rows=None):
    x, p = worlds[dim][:2]
    ix = va.Index(dim, dtype, metric)
    if reserve:
        ix.reserve(len(x) + 300)
    ix.set_id_offset(off)
    ix.add(x if rows is None else rows)
    if keys:
        ix.set_keys(off, np.arange(len(x), dtype=np.uint64) + np.uint64(77000))
    ix.delete(p["dead"] + np.uint64(off))
    return ix, p


def check_planted(out, at, p, dtype, metric, off=OFF):
    """What the planted structure says, whatever the model says."""
    f = lambda name, j=0: int(out[at[name][j]])
    assert f("big") == p["big"][0] + off and f("again", 1) == p["big"][0] + off
    assert f("first_dead") == p["first_dead"][1] + off
    assert f("all_dead") == f("all_dead", 1) == f("again", 6) == NONE
    assert f("two_x") == f("again", 2) == (p["solo"][0] + off if metric == "cosine" else NONE)
    if metric != "cosine":
        assert f("twin") == (p["z"][0] + off if dtype == "bf16" else NONE)
        assert f("rounded") == (p["rounded"][0] + off if dtype == "bf16" else p["rounded"][1] + off)
        assert f("scaled") == p["scaled"][1] + off
    else:
        assert f("scaled") == f("scaled", 1) == p["scaled"][0] + off
    assert [f("near", j) for j in range(4)] == [NONE] * 4 and f("again", 5) == NONE
    assert f("z") == p["z"][0] + off and f("edge") == p["edge"][0] + off
    assert [f("solo", j) for j in range(len(p["solo"]))] == [r + off for r in p["solo"]]
    assert all(int(out[i]) == NONE for i in at["new_a"] + at["new_b"]) and f("again", 0) == f("again", 3) == f("again", 7) == NONE


def same_state(ix, ctl, rq, tmp_path, what):
    """Two handles are one through the ABI: count, stored bits, a search's ids and score bits, eps_bound, snapshot bytes."""
    assert ix.count == ctl.count and ix.live_count() == ctl.live_count(), what
    assert np.array_equal(bits(ix.get_rows(0, ix.count)), bits(ctl.get_rows(0, ctl.count))), what
    assert_same(*ix.search(rq, 10), *ctl.search(rq, 10), what)
    assert bits(np.float32(ix.last_stats()["eps_bound"])) == bits(np.float32(ctl.last_stats()["eps_bound"])), what
    a, b = tmp_path / "a.vrod", tmp_path / "b.vrod"
    ix.save(a)
    ctl.save(b)
    assert a.read_bytes() == b.read_bytes(), what


def queries(worlds, dim, inputs):
    rq = np.random.default_rng(11).standard_normal((32, dim)).astype(np.float32)
    rq[0], rq[1], rq[2] = worlds[dim][0][worlds[dim][1]["big"][0]], inputs[0], inputs[-2]
    return rq


# ---------------------------------------------------------------- 1: find_rows against the model
@pytest.mark.parametrize("dtype,metric,dim", CASES + LONG)
def test_find_rows_equals_the_model(va, O, worlds, dtype, metric, dim):
    x, _, inputs, at = worlds[dim]
    ix, p = filled(va, worlds, dtype, metric, dim)
    with ix:
        want, wst, _ = rowfind_model.of_handle(O, ix, dtype, metric, inputs, p["dead"] + np.uint64(OFF))
        got, st = ix.find_rows(inputs, stats=True)
        print(dtype, metric, dim, st)
        assert got.dtype == np.uint64 and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert exact(st) == wst and st["appended"] == 0 and st["batches"] == 1 and st["slots"] >= max(1024, 4 * len(inputs)) and st["max_probe"] >= 1
        assert st["found"] > 15 and st["repeats"] >= 3 and st["found"] + st["repeats"] < st["rows"] == len(inputs)
        check_planted(got, at, p, dtype, metric)
        again, st2 = ix.find_rows(inputs, stats=True)
        assert np.array_equal(again, got) and exact(st2) == exact(st)            # a function of the handle's state and the inputs alone
        narrow, nst = ix.find_rows(inputs, narrow_hash=True, stats=True)
        assert np.array_equal(narrow, want) and exact(nst) == wst
        small, sst = ix.find_rows(inputs, small_batch=True, stats=True)          # repeats across batches go through the side corpus
        assert np.array_equal(small, want) and exact(sst) == wst and sst["batches"] == -(-len(inputs) // 96) == 2
        both = ix.find_rows(inputs, small_batch=True, narrow_hash=True)
        assert np.array_equal(both, want)
        _, only = ix.find_rows(inputs[:0], stats=True)                           # n == 0: zero stats
        assert only == {k: 0 for k in only}
        assert ix.count == N if dim != 4099 else ix.count == 40


# ---------------------------------------------------------------- 2: the narrow hash meets
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 33), ("f32", "l2", 8), ("bf16", "l2", 768)])
def test_narrow_hash_gives_the_same_ids_through_collisions(va, O, dtype, metric, dim):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((300, dim)).astype(np.float32)
    inputs = np.concatenate([rng.standard_normal((300, dim)).astype(np.float32), x[[7, 299, 7]]])   # 300 distinct new rows and a few copies
    with va.Index(dim, dtype, metric) as ix:
        ix.add(x)
        want, wst, _ = rowfind_model.of_handle(O, ix, dtype, metric, inputs)
        assert wst == {"rows": 303, "found": 3, "repeats": 0, "appended": 0}
        wide, st = ix.find_rows(inputs, stats=True)
        narrow, nst = ix.find_rows(inputs, narrow_hash=True, stats=True)
        print(dtype, metric, dim, st, nst)
        assert np.array_equal(wide, want) and np.array_equal(narrow, want) and exact(st) == exact(nst) == wst
        assert nst["compare_misses"] > 0                                         # 300 distinct inputs over 256 hash values: two must meet in the batch's table
        got, ast = ix.add_unique(inputs, narrow_hash=True, small_batch=True, stats=True)
        assert exact(ast) == {"rows": 303, "found": 3, "repeats": 0, "appended": 300} and ix.count == 600 and ast["compare_misses"] > 0
        assert np.array_equal(got[:300], np.arange(300, 600, dtype=np.uint64)) and got[300:].tolist() == [7, 299, 7]


# ---------------------------------------------------------------- 3: the filter, a snapshot, compaction
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 768), ("f32", "l2", 33), ("bf16", "l2", 8)])
def test_filter_snapshot_and_compaction(va, O, worlds, dtype, metric, dim, tmp_path):
    x, _, inputs, at = worlds[dim]
    ix, p = filled(va, worlds, dtype, metric, dim, keys=True)
    with ix:
        before, after = tmp_path / "before.vrod", tmp_path / "after.vrod"
        ix.save(before)
        got, st = ix.find_rows(inputs, stats=True)
        ix.find_rows(inputs, small_batch=True, narrow_hash=True)
        ix.save(after)
        assert before.read_bytes() == after.read_bytes()                         # the handle is not changed in any observable way
        allow = np.ones(N, bool)
        allow[(got[got != ID_NONE] - np.uint64(OFF)).astype(np.int64)] = False   # the filter excludes every match: it is not consulted
        ix.set_filter(allow)
        filtered, fst = ix.find_rows(inputs, stats=True)
        assert np.array_equal(filtered, got) and exact(fst) == exact(st) and ix.filter_count() < ix.live_count()
        ix.set_filter(None)
        new_ids = ix.compact()
        want, wst, _ = rowfind_model.of_handle(O, ix, dtype, metric, inputs)
        moved, mst = ix.find_rows(inputs, stats=True)
        assert np.array_equal(moved, want) and exact(mst) == wst == exact(st)
        hit = got != ID_NONE
        assert np.array_equal(moved[hit], new_ids[(got[hit] - np.uint64(OFF)).astype(np.int64)]) and np.all(moved[~hit] == ID_NONE)   # the renumbered ids


# ---------------------------------------------------------------- 4: the device forms
@pytest.mark.parametrize("dtype,metric,dim,src", [("bf16", "cosine", 768, "float16"), ("f32", "l2", 33, "bfloat16"), ("bf16", "l2", 8, "float16"),
                                                  ("f32", "cosine", 33, "float32")])
def test_device_forms(va, O, worlds, dtype, metric, dim, src, tmp_path):
    import torch
    tt = getattr(torch, src)
    widen = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(tt).float().numpy()   # what the source type keeps of a row
    x, _, inputs, at = worlds[dim]
    xs, ins = widen(x), widen(inputs)
    n, stride = len(ins), dim + 3
    flat = torch.full((n * stride + 9,), 3.0, dtype=tt, device="cuda")
    view = flat[1:1 + n * stride].view(n, stride)[:, :dim]                       # a base one element off: the ingest's word path
    view.copy_(torch.from_numpy(ins).to(tt))
    assert view.data_ptr() % 16 != 0 and view.stride(0) == stride
    ix, p = filled(va, worlds, dtype, metric, dim, rows=xs)
    ctl, _ = filled(va, worlds, dtype, metric, dim, rows=xs)
    with ix, ctl:
        want, wst, _ = rowfind_model.of_handle(O, ix, dtype, metric, ins, p["dead"] + np.uint64(OFF))
        buf = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        out, st = ix.find_rows_device(view, out_ids=buf)
        assert out is buf and np.array_equal(buf[:n].cpu().numpy().view(np.uint64), want) and exact(st) == wst
        assert int(buf[n]) == 0x5A5A5A5A                                         # the guard past n is untouched
        assert np.array_equal(ix.find_rows(ins), want)                           # the host form of the widened values
        out, sst = ix.find_rows_device(view, small_batch=True, narrow_hash=True)
        assert np.array_equal(out[:n].cpu().numpy().view(np.uint64), want) and exact(sst) == wst and sst["batches"] == 2
        assert int(want[at["big"][0]]) == p["big"][0] + OFF and int(want[at["first_dead"][0]]) == p["first_dead"][1] + OFF
        want, wst, app = rowfind_model.of_handle(O, ix, dtype, metric, ins, p["dead"] + np.uint64(OFF), append=True)
        out, ast = ix.add_unique_device(view, out_ids=buf)
        assert np.array_equal(buf[:n].cpu().numpy().view(np.uint64), want) and exact(ast) == wst and int(buf[n]) == 0x5A5A5A5A
        ctl.add(ins[app])
        same_state(ix, ctl, queries(worlds, dim, ins), tmp_path, "add_unique_device")
        assert bool((flat[1 + n * stride:] == 3.0).all()) and float(flat[0]) == 3.0


# ---------------------------------------------------------------- 5: add_unique is add() of the appended inputs
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 768), ("f32", "l2", 33), ("bf16", "l2", 8), ("f32", "cosine", 8), ("f32", "ip", 768),
                                              ("bf16", "cosine", 33), ("f32", "l2", 4099)])
def test_add_unique_is_add_of_the_appended_inputs(va, O, worlds, dtype, metric, dim, tmp_path):
    x, _, inputs, at = worlds[dim]
    count = len(x)
    ix, p = filled(va, worlds, dtype, metric, dim, keys=True)
    ctl, _ = filled(va, worlds, dtype, metric, dim, keys=True)
    with ix, ctl:
        dups = ix.find_duplicates(stats=True)[1]["duplicates"]
        keyed = ix.key_stats()["keyed_live"]
        want, wst, app = rowfind_model.of_handle(O, ix, dtype, metric, inputs, p["dead"] + np.uint64(OFF), append=True)
        got, st = ix.add_unique(inputs, stats=True)
        print(dtype, metric, dim, st)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert exact(st) == wst and st["appended"] == len(app) == st["rows"] - st["found"] - st["repeats"] > 90
        assert np.array_equal(got[app], np.arange(count, count + len(app), dtype=np.uint64) + np.uint64(OFF))   # the next ids, in call order
        ctl.add(inputs[app])
        same_state(ix, ctl, queries(worlds, dim, inputs), tmp_path, "add_unique")
        assert ix.find_duplicates(stats=True)[1]["duplicates"] == dups           # nothing it appended has a copy
        assert ix.key_stats()["keyed_live"] == keyed and np.all(ix.get_keys(OFF + count, len(app)) == ID_NONE)   # the appended rows are keyless
        again, st2 = ix.add_unique(inputs, stats=True)                           # the same batch again appends nothing
        assert np.array_equal(again, got) and st2["appended"] == 0 and st2["found"] + st2["repeats"] == st2["rows"] and ix.count == ctl.count
        assert np.array_equal(ix.find_rows(inputs), got)
        same_state(ix, ctl, queries(worlds, dim, inputs), tmp_path, "add_unique twice")


# ---------------------------------------------------------------- 6: batches that see each other's appends; crossing the capacity
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 768), ("f32", "l2", 33), ("bf16", "l2", 8)])
def test_small_batches_cross_the_capacity_and_see_earlier_appends(va, O, worlds, dtype, metric, dim, tmp_path):
    x, _, batch, at = worlds[dim]
    n = 2 * 96 + 5
    rng = np.random.default_rng(3 * dim)
    inputs = rng.standard_normal((n, dim)).astype(np.float32)
    inputs[40], inputs[100], inputs[150] = x[worlds[dim][1]["big"][9]], x[worlds[dim][1]["edge"][0]], 2.0 * x[worlds[dim][1]["solo"][1]]
    inputs[2 * 96 + 2] = inputs[3]                                               # the third batch repeats a NEW input of the first
    inputs[96 + 7], inputs[96 + 8], inputs[2 * 96 + 4] = inputs[95], inputs[96 + 1], inputs[96 + 1]
    ix, p = filled(va, worlds, dtype, metric, dim, reserve=False)                # the capacity is the count rounded up: 300 new rows cross it
    ctl, _ = filled(va, worlds, dtype, metric, dim, reserve=False)
    with ix, ctl:
        want, wst, _ = rowfind_model.of_handle(O, ix, dtype, metric, inputs, p["dead"] + np.uint64(OFF))
        got, st = ix.find_rows(inputs, small_batch=True, stats=True)             # nothing is appended: the side corpus resolves the repeats
        assert np.array_equal(got, want) and exact(st) == wst and st["batches"] == 3 and st["repeats"] >= 4
        want, wst, app = rowfind_model.of_handle(O, ix, dtype, metric, inputs, p["dead"] + np.uint64(OFF), append=True)
        got, st = ix.add_unique(inputs, small_batch=True, stats=True)
        assert np.array_equal(got, want) and exact(st) == wst and st["batches"] == 3
        assert got[2 * 96 + 2] == got[3] == np.uint64(OFF + N + 3) and got[2 * 96 + 4] == got[96 + 8] == got[96 + 1] and got[96 + 7] == got[95]
        assert ix.count == N + len(app) and len(app) >= n - 8
        ctl.add(inputs[app])
        same_state(ix, ctl, queries(worlds, dim, inputs), tmp_path, "small batches")
        assert ix.add_unique(inputs, small_batch=True, stats=True)[1]["appended"] == 0 and ix.count == ctl.count
        more = rng.standard_normal((150, dim)).astype(np.float32)                # this call takes the count past 512, the capacity of both handles
        more[120] = more[20]
        assert ix.count < 512 < ix.count + 140
        got, st = ix.add_unique(more, small_batch=True, stats=True)
        assert exact(st) == {"rows": 150, "found": 0, "repeats": 1, "appended": 149} and got[120] == got[20]
        ctl.add(np.delete(more, 120, axis=0))
        same_state(ix, ctl, queries(worlds, dim, inputs), tmp_path, "across the capacity")


def test_an_empty_handle_deduplicates_the_call(va, O, worlds, tmp_path):
    x, _, inputs, at = worlds[33]
    with va.Index(33, "bf16", "cosine") as ix, va.Index(33, "bf16", "cosine") as ctl:
        got, st = ix.find_rows(inputs, stats=True)
        assert np.all(got == ID_NONE) and st["found"] == 0 and st["repeats"] > 0
        want, wst, app = rowfind_model.of_handle(O, ix, "bf16", "cosine", inputs, append=True)
        got, ast = ix.add_unique(inputs, stats=True)
        assert np.array_equal(got, want) and exact(ast) == wst and ast["found"] == 0 and ast["repeats"] == st["repeats"] and ix.count == len(app)
        ctl.add(inputs[app])
        same_state(ix, ctl, queries(worlds, 33, inputs), tmp_path, "empty handle")
        assert ix.find_duplicates(stats=True)[1]["duplicates"] == 0


# ---------------------------------------------------------------- 7: refusals
def test_refusals_leave_outputs_and_handle_alone(va, worlds):
    import torch
    from vrod_amd._lib import RowfindStats
    L = va.load()
    x, _, inputs, at = worlds[33]
    ix, p = filled(va, worlds, "bf16", "cosine", 33)
    n = 2 * 96 + 5
    bad = np.ascontiguousarray(np.random.default_rng(1).standard_normal((n, 33)).astype(np.float32))
    bad[n - 2, 17] = np.nan                                                      # in the last lookup batch
    rq = queries(worlds, 33, inputs)
    vp = C.c_void_p

    def refused(h, code, rows, flags=0, device=False):
        """Both calls, in one form, answer `code`; ids and stats are as they were."""
        out = np.full(n, 7, np.uint64)
        st = RowfindStats(*([9] * 8))
        for name in ("vrod_index_find_rows", "vrod_index_add_unique"):
            if device:
                d = torch.full((n,), 7, dtype=torch.int64, device="cuda")
                t = torch.from_numpy(rows).cuda()
                assert getattr(L, name + "_device")(h._h, t.data_ptr(), 0, 33, n, flags, d.data_ptr(), C.byref(st), None) == code, name
                assert bool((d == 7).all())
            else:
                assert getattr(L, name)(h._h, rows.ctypes.data_as(vp), n, flags, out.ctypes.data_as(vp), C.byref(st)) == code, name
        assert np.all(out == 7) and all(getattr(st, f) == 9 for f, _ in RowfindStats._fields_)

    with ix:
        ids0, sc0 = ix.search(rq, 10)
        eps0, rows0, count0 = ix.last_stats()["eps_bound"], ix.get_rows(0, N), ix.count
        for device in (False, True):
            refused(ix, ERR_INVALID_VALUE, bad, 0x40000000, device)              # under SMALL_BATCH: two batches are clean, the third is not
            refused(ix, ERR_INVALID_VALUE, bad, 0, device)
            for flags in (1, 2, 0x20000000, 0xC0000001, 0xFFFFFFFF):             # unknown flag bits
                refused(ix, ERR_INVALID_ARG, bad, flags, device)
        big = bad.copy()
        big[n - 2, 17] = np.inf
        big[5] *= 1000.0                                                         # a clean row with a large norm in front of the bad one
        refused(ix, ERR_INVALID_VALUE, big, 0x40000000)
        assert ix.count == count0 and ix.live_count() == count0 - len(p["dead"]) and np.array_equal(bits(ix.get_rows(0, N)), bits(rows0))
        ids1, sc1 = ix.search(rq, 10)
        assert_same(ids1, sc1, ids0, sc0, "after the refusals")
        assert bits(np.float32(ix.last_stats()["eps_bound"])) == bits(np.float32(eps0))
        oi = torch.empty((4, 10), dtype=torch.int64, device="cuda")
        osc = torch.empty((4, 10), dtype=torch.float32, device="cuda")
        ix.search_begin_synthetic_device(2, 0, 4, 10, oi, osc)                   # a pending search
        clean = bad.copy()
        clean[n - 2, 17], clean[0] = 0.5, x[p["big"][0]]
        for device in (False, True):
            refused(ix, ERR_INVALID_ARG, clean, 0, device)
        ix.search_end()
        assert ix.count == count0
        got, st = ix.add_unique(clean, stats=True)                               # and the handle still works
        assert st["appended"] > 0 and ix.count == count0 + st["appended"]
    with va.Index(33, "bf16", "cosine", devices=[0, 0]) as two:                  # a multi-device handle
        two.add(x)
        for device in (False, True):
            refused(two, ERR_UNSUPPORTED, clean, 0, device)
        assert two.count == N
