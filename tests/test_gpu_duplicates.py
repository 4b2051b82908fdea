"""GPU tests of duplicate-row detection (vrod_index_find_duplicates, _find_duplicates_device, _delete_duplicates) against
dup_model, which groups the rows get_rows reads back by their bytes.

The corpus is the smallest at which the passes can go wrong: kDupRowsPerGroup (256) + 37 rows, so two work-groups and a
last wave that is partial, added after reserve(N + 300) so that the capacity exceeds the count; dims 8 (one 16-byte unit
per bf16 row, one lane a row), 33 (the word path, a half-filled last word on bf16) and 768 (the whole wave a row), and 40
rows of dim 4099 for long rows through the word path.  Random rows carry planted structure (see `planted`).  Everything
is exact -- maps, the four exact stats, ids and score bits -- except the three diagnostics, of which only
compare_misses > 0 under the narrow hash is asserted (300 distinct rows over 256 hash values must meet).
"""
import ctypes as C
import os

import numpy as np
import pytest

import dup_model
from dup_model import ID_NONE, exact
from support import va, assert_same, bits  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS_PER_GROUP = 256                                 # dup_plan.h kDupRowsPerGroup
N = ROWS_PER_GROUP + 37
G = ROWS_PER_GROUP
OFF = 5000
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 6
CASES = [(dt, me, d) for dt in ("bf16", "f32") for me in ("cosine", "l2") for d in (8, 33, 768)]


def test_the_shape_is_the_one_the_passes_cut():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vrod_amd", "csrc", "dup_plan.h")).read()
    assert f"constexpr uint32_t kDupRowsPerGroup = {ROWS_PER_GROUP};" in text
    assert -(-N // ROWS_PER_GROUP) == 2 and (N - ROWS_PER_GROUP) % 64 and N % 32
    assert -(-(N + 300) // 256) * 256 > N + 64                                   # the capacity reaches past the last wave


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
    p["lone"] = take(3)                                                          # all but the middle one deleted: it is its own first
    x[p["lone"]] = x[p["lone"][0]]
    base = bf16_exact(rng.standard_normal(dim).astype(np.float32))
    base[2] = 0.0
    base[1], base[dim - 2] = np.float32(0.75), np.float32(-1.25)
    p["near"] = take(6)                                                          # a class of two and four rows that are almost it
    b0, b1, last, first, sign, swap = p["near"]
    x[[b0, b1, last, first, sign, swap]] = base
    x[last, -1] *= np.float32(1.5)                                               # only the last element differs
    x[first, 0] *= np.float32(1.5)                                               # only the first
    x[sign, 2] = np.float32(-0.0)                                                # only the sign of a zero
    x[swap, [1, dim - 2]] = base[[dim - 2, 1]]                                   # two elements swapped
    p["scaled"] = take(2)                                                        # a row and twice that row: one class under cosine
    x[p["scaled"][1]] = 2.0 * x[p["scaled"][0]]
    p["rounded"] = take(2)                                                       # two fp32 rows that round to one bf16 row
    x[p["rounded"][0]] = bf16_exact(x[p["rounded"][0]])
    x[p["rounded"][1]] = x[p["rounded"][0]] * np.float32(1 + 2.0 ** -12)
    assert not np.array_equal(x[p["rounded"][0]], x[p["rounded"][1]])
    dead = [p["first_dead"][0], p["lone"][0], p["lone"][2]]
    dead += [int(r) for r in rng.choice(free, min(60, len(free) // 2), replace=False)]   # the random deletes leave the planted rows alone
    p["dead"] = np.array(sorted(dead), np.uint64)
    return x, p


@pytest.fixture(scope="module")
def worlds():
    w = {d: planted(d) for d in (8, 33, 768)}
    w[4099] = planted(4099, n=40)
    return w


def filled(va, worlds, dtype, metric, dim, off=0, labels=None, keys=False):
    x, p = worlds[dim]
    ix = va.Index(dim, dtype, metric)
    ix.reserve(len(x) + 300)
    ix.set_id_offset(off)
    ix.add(x)
    if labels is not None:
        ix.set_labels(off, labels)
    if keys:
        ix.set_keys(off, np.arange(len(x), dtype=np.uint64) + np.uint64(77000))
    ix.delete(p["dead"] + np.uint64(off))
    return ix, p


def check_planted(out, p, dtype, metric, off=0):
    """What the planted structure says, whatever the model says."""
    f = lambda r: int(out[r]) - off
    assert f(p["edge"][1]) == p["edge"][0] == f(p["edge"][0])
    assert all(f(r) == p["big"][0] for r in p["big"])
    assert [int(out[r]) for r in p["first_dead"]] == [int(ID_NONE)] + [p["first_dead"][1] + off] * 3
    assert [int(out[r]) for r in p["lone"]] == [int(ID_NONE), p["lone"][1] + off, int(ID_NONE)]
    b0, b1, last, first, sign, swap = p["near"]
    assert f(b0) == f(b1) == b0 and [f(r) for r in (last, first, sign, swap)] == [last, first, sign, swap]
    if dtype == "bf16" and metric == "l2":
        assert f(p["rounded"][1]) == p["rounded"][0]                             # equality after rounding
    if dtype == "f32" and metric == "l2":
        assert f(p["rounded"][1]) == p["rounded"][1] and f(p["scaled"][1]) == p["scaled"][1]


# ---------------------------------------------------------------- 1: the map and the exact stats
@pytest.mark.parametrize("dtype,metric,dim", CASES + [("bf16", "cosine", 4099), ("f32", "l2", 4099)])
def test_map_and_stats_equal_the_model(va, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim)
    with ix:
        want, wst = dup_model.of_handle(ix, p["dead"])
        got, st = ix.find_duplicates(stats=True)
        print(dtype, metric, dim, st)
        assert got.dtype == np.uint64 and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        assert exact(st) == wst and st["duplicates"] == st["live"] - st["classes"] and st["live"] == ix.live_count()
        assert st["largest_class"] == len(p["big"]) and st["slots"] >= max(1024, 4 * st["live"]) and st["max_probe"] >= 1
        check_planted(got, p, dtype, metric)
        if metric == "cosine":                                                   # x and 2x: asserted from the stored rows, then relied on
            a, b = (ix.get_rows(r, 1) for r in p["scaled"])
            assert np.array_equal(bits(a), bits(b)) and got[p["scaled"][1]] == p["scaled"][0]
        again, st2 = ix.find_duplicates(stats=True)
        assert np.array_equal(again, got) and exact(st2) == exact(st)            # a function of the handle's state alone
        only, st3 = ix.find_duplicates(stats=True, within_label=True)            # a handle without labels: the flag changes nothing
        assert np.array_equal(only, got) and exact(st3) == exact(st)


# ---------------------------------------------------------------- 2: the narrow hash
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 33), ("f32", "l2", 8), ("bf16", "l2", 768)])
def test_narrow_hash_gives_the_same_result_through_collisions(va, dtype, metric, dim):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((300 + 6, dim)).astype(np.float32)
    x[300:303], x[303:] = x[7], x[299]                                           # 300 distinct rows and a few copies
    with va.Index(dim, dtype, metric) as ix:
        ix.add(x)
        want, wst = dup_model.of_handle(ix)
        assert wst["classes"] == 300 and wst["largest_class"] == 4
        wide, st = ix.find_duplicates(stats=True)
        narrow, nst = ix.find_duplicates(narrow_hash=True, stats=True)
        print(dtype, metric, dim, st, nst)
        assert np.array_equal(wide, want) and np.array_equal(narrow, want)
        assert exact(st) == exact(nst) == wst
        assert nst["compare_misses"] > 0                                         # 300 distinct rows over 256 hash values: two must meet
        assert np.array_equal(ix.find_duplicates(narrow_hash=True, within_label=True), want)


# ---------------------------------------------------------------- 3: the ties a search cannot separate
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 768), ("f32", "l2", 8), ("bf16", "l2", 33), ("f32", "cosine", 33)])
def test_a_class_is_one_tie_for_every_search(va, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim)
    with ix:
        out = ix.find_duplicates()
        first = int(out[p["big"][7]])
        cls = np.flatnonzero(out == np.uint64(first))                            # the class as find_duplicates reports it
        assert cls.size == 100 and cls.tolist() == p["big"]
        ids, sc = ix.search(worlds[dim][0][first][None], 102)
        assert ids[0, :100].tolist() == cls.tolist()                             # ascending: ties go to the smaller id
        assert np.unique(bits(sc[0, :100])).size == 1 and bits(sc[0, 100]) != bits(sc[0, 0])


# ---------------------------------------------------------------- 4: delete_duplicates
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 768), ("f32", "l2", 33), ("bf16", "l2", 8)])
def test_delete_duplicates_is_delete_of_the_non_first_ids(va, worlds, dtype, metric, dim):
    ix, p = filled(va, worlds, dtype, metric, dim, off=OFF, keys=True)
    model, _ = filled(va, worlds, dtype, metric, dim, off=OFF, keys=True)
    allow = np.random.default_rng(5).random(N) < 0.8
    rq = np.random.default_rng(6).standard_normal((6, dim)).astype(np.float32)
    rq[0] = worlds[dim][0][p["big"][0]]
    with ix, model:
        for h in (ix, model):
            h.set_filter(allow)
        out, st = ix.find_duplicates(stats=True)
        ids = np.arange(N, dtype=np.uint64) + np.uint64(OFF)
        gone = ids[(out != ID_NONE) & (out != ids)]
        assert gone.size == st["duplicates"] > 100
        model.delete(gone)
        assert ix.delete_duplicates() == st["duplicates"]
        assert (ix.live_count(), ix.filter_count()) == (model.live_count(), model.filter_count())
        assert ix.filter_count() < ix.live_count() == st["classes"]
        assert_same(*ix.search(rq, 10), *model.search(rq, 10), "after delete_duplicates")
        keys = gone - np.uint64(OFF) + np.uint64(77000)
        assert np.array_equal(ix.find_keys(keys), model.find_keys(keys)) and np.all(ix.find_keys(keys) == ID_NONE)
        kept = ids[out == ids] - np.uint64(OFF) + np.uint64(77000)
        assert np.array_equal(ix.find_keys(kept), model.find_keys(kept)) and np.array_equal(ix.find_keys(kept), ids[out == ids])
        out2, st2 = ix.find_duplicates(stats=True)
        assert st2["duplicates"] == 0 and st2["largest_class"] == 1 and st2["live"] == st2["classes"] == st["classes"]
        assert np.array_equal(out2[out2 != ID_NONE], ids[out == ids])
        assert ix.delete_duplicates() == 0 and ix.live_count() == st["classes"]
        ix.compact()
        after = ix.find_duplicates()
        assert after.size == st["classes"] and np.array_equal(after, np.arange(after.size, dtype=np.uint64) + np.uint64(OFF))   # the identity


# ---------------------------------------------------------------- 5: within a label
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 33), ("f32", "l2", 768)])
def test_within_label_splits_a_class_that_spans_two_labels(va, worlds, dtype, metric, dim):
    _, p = worlds[dim]
    labels = np.full(N, 7, np.uint32)
    other = p["big"][40:]                                                        # the big class spans labels 7 and 0xFFFFFFFF
    labels[other] = 0xFFFFFFFF
    ix, _ = filled(va, worlds, dtype, metric, dim, labels=labels)
    with ix:
        plain, st = ix.find_duplicates(stats=True)
        want, wst = dup_model.of_handle(ix, p["dead"])
        assert np.array_equal(plain, want) and exact(st) == wst                  # without the flag the labels are not read
        got, lst = ix.find_duplicates(within_label=True, stats=True)
        want, wst = dup_model.of_handle(ix, p["dead"], within_label=True, labels=labels)
        assert np.array_equal(got, want) and exact(lst) == wst
        assert lst["classes"] == st["classes"] + 1 and lst["largest_class"] == 60
        assert np.all(got[other] == np.uint64(other[0])) and np.all(got[p["big"][:40]] == np.uint64(p["big"][0]))
        rest = np.setdiff1d(np.arange(N), other)
        assert np.array_equal(got[rest], plain[rest])                            # the rest is unchanged
        assert np.array_equal(ix.find_duplicates(within_label=True, narrow_hash=True), got)
        assert ix.delete_duplicates(within_label=True) == lst["duplicates"] and ix.live_count() == lst["classes"]
        assert ix.find_duplicates(stats=True)[1]["duplicates"] == 1              # the two halves of the big class are left


# ---------------------------------------------------------------- 6: life cycle
@pytest.mark.parametrize("dtype,metric,dim,off", [("bf16", "cosine", 8, 0), ("f32", "l2", 33, OFF), ("bf16", "l2", 768, OFF)])
def test_updates_growth_and_the_id_offset(va, worlds, dtype, metric, dim, off):
    x, p = worlds[dim]
    ix, _ = filled(va, worlds, dtype, metric, dim)
    o = np.uint64(off)
    with ix:
        ix.set_id_offset(off)
        dead = p["dead"] + o
        solo = [r for r in range(N) if r not in set(p["dead"].tolist()) | set(sum((p[k] for k in ("edge", "big", "first_dead", "lone", "near", "scaled", "rounded")), []))]
        a, b = solo[0], solo[-1]
        out = ix.find_duplicates()
        assert out[a] == a + o and out[b] == b + o and np.array_equal(out, dup_model.of_handle(ix, dead)[0])
        ix.update([b + off], x[a][None])                                         # an update to another row's vector joins them
        out = ix.find_duplicates()
        assert out[b] == out[a] == a + o and np.array_equal(out, dup_model.of_handle(ix, dead)[0])
        member = p["big"][50]
        ix.update([member + off], np.random.default_rng(9).standard_normal((1, dim)).astype(np.float32))   # a fresh vector splits it off
        out, st = ix.find_duplicates(stats=True)
        assert out[member] == member + o and st["largest_class"] == 99 and np.array_equal(out, dup_model.of_handle(ix, dead)[0])
        more = np.random.default_rng(10).standard_normal((700, dim)).astype(np.float32)   # past reserve(N + 300): the allocation grows
        more[5], more[699] = x[a], x[p["big"][0]]
        ix.add(more)
        out, st = ix.find_duplicates(stats=True)
        want, wst = dup_model.of_handle(ix, dead)
        assert out.size == N + 700 and np.array_equal(out, want) and exact(st) == wst
        assert out[N + 5] == a + o and out[N + 699] == p["big"][0] + o and st["largest_class"] == 100
        assert out[p["dead"][0]] == ID_NONE


# ---------------------------------------------------------------- 7: the device form
@pytest.mark.parametrize("dtype,metric,dim", [("bf16", "cosine", 768), ("f32", "l2", 33)])
def test_device_form_writes_the_same_map(va, worlds, dtype, metric, dim):
    import torch
    ix, p = filled(va, worlds, dtype, metric, dim, off=OFF)
    with ix:
        want, wst = ix.find_duplicates(stats=True)
        buf = torch.full((N + 1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        out, st = ix.find_duplicates_device(out_first=buf)
        assert out is buf and np.array_equal(buf[:N].cpu().numpy().view(np.uint64), want) and exact(st) == exact(wst)
        assert int(buf[N]) == 0x5A5A5A5A                                         # the guard past count is untouched
        fresh, _ = ix.find_duplicates_device(narrow_hash=True)
        assert np.array_equal(fresh[:N].cpu().numpy().view(np.uint64), want)


# ---------------------------------------------------------------- 8: refusals and empty handles
def test_refusals_leave_the_outputs_alone(va, worlds):
    import torch
    from vrod_amd._lib import DupStats
    L = va.load()
    ix, p = filled(va, worlds, "bf16", "cosine", 8)

    def refused(h, code, flags=0, device=False):
        """Both forms of find and the delete answer `code`; the map, the stats and the count are as they were."""
        out = np.full(N + 8, 7, np.uint64)
        st = DupStats(*([9] * 7))
        n = C.c_uint64(7)
        if device:
            d = torch.full((N + 8,), 7, dtype=torch.int64, device="cuda")
            assert L.vrod_index_find_duplicates_device(h._h, flags, d.data_ptr(), N, C.byref(st), None) == code
            assert bool((d == 7).all())
        else:
            assert L.vrod_index_find_duplicates(h._h, flags, out.ctypes.data_as(C.c_void_p), N, C.byref(st)) == code
        assert L.vrod_index_delete_duplicates(h._h, flags, C.byref(n)) == code
        assert np.all(out == 7) and all(getattr(st, f) == 9 for f, _ in DupStats._fields_)
        return n.value

    with ix:
        live = ix.live_count()
        for device in (False, True):
            for bad_len in (0, N - 1, N + 1, N + 8):
                st = DupStats(*([9] * 7))
                out = np.full(N + 8, 7, np.uint64)
                d = torch.full((N + 8,), 7, dtype=torch.int64, device="cuda")
                if device:
                    rc = L.vrod_index_find_duplicates_device(ix._h, 0, d.data_ptr(), bad_len, C.byref(st), None)
                else:
                    rc = L.vrod_index_find_duplicates(ix._h, 0, out.ctypes.data_as(C.c_void_p), bad_len, C.byref(st))
                assert rc == ERR_INVALID_ARG and np.all(out == 7) and bool((d == 7).all()) and st.live == 9
            st = DupStats(*([9] * 7))
            assert L.vrod_index_find_duplicates(ix._h, 0, None, N, C.byref(st)) == ERR_INVALID_ARG and st.live == 9   # a length without a map
            for flags in (2, 4, 0x40000000, 0x80000002, 0xFFFFFFFF):             # unknown flag bits
                assert refused(ix, ERR_INVALID_ARG, flags, device=device) == 7
        assert ix.live_count() == live
        oi = torch.empty((4, 10), dtype=torch.int64, device="cuda")
        osc = torch.empty((4, 10), dtype=torch.float32, device="cuda")
        ix.search_begin_synthetic_device(2, 0, 4, 10, oi, osc)                   # a pending search
        for device in (False, True):
            assert refused(ix, ERR_INVALID_ARG, device=device) == 7
        st = DupStats(*([9] * 7))
        assert L.vrod_index_find_duplicates(ix._h, 0, None, 0, C.byref(st)) == ERR_INVALID_ARG and st.live == 9
        ix.search_end()
        assert ix.live_count() == live and ix.find_duplicates(stats=True)[1]["live"] == live
    with va.Index(8, "bf16", "cosine", devices=[0, 0]) as two:                   # a multi-device handle
        two.add(worlds[8][0])
        for device in (False, True):
            assert refused(two, ERR_UNSUPPORTED, device=device) == 7
        assert two.live_count() == N


def test_empty_handles_give_zero_stats(va, worlds):
    zero = {k: 0 for k in ("live", "classes", "duplicates", "largest_class", "slots", "max_probe", "compare_misses")}
    with va.Index(8, "f32", "l2") as empty:
        for _ in range(2):
            out, st = empty.find_duplicates(stats=True)
            assert out.size == 0 and st == zero and empty.delete_duplicates() == 0
            out, st = empty.find_duplicates_device()
            assert st == zero
            empty.reserve(500)
    with va.Index(33, "bf16", "cosine") as ix:                                   # every row deleted
        ix.add(worlds[33][0])
        ix.delete(np.arange(N, dtype=np.uint64))
        out, st = ix.find_duplicates(stats=True, within_label=True)
        assert out.size == N and np.all(out == ID_NONE) and st == zero
        d, st = ix.find_duplicates_device()
        assert np.all(d[:N].cpu().numpy().view(np.uint64) == ID_NONE) and st == zero
        assert ix.delete_duplicates() == 0 and ix.live_count() == 0
