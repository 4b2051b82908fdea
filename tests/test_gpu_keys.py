"""GPU tests of the row keys (vrod_index_set_keys, _find_keys, _ids_to_keys, _delete_keys, _upsert, _key_stats) against
keys_model.KeysModel, the plain-Python statement of include/vrod.h "Row keys".

Keys are integers: every comparison is exact.  Where a search is involved the results are compared bit for bit, with the
model (the CPU oracle over the rows the model holds) or with a second handle that received the equivalent update and add
calls.  dim 8 and a few hundred rows: the table starts at 1024 slots, so 300 to 800 keys reach growth, rebuilds and stale
slots; vrod_key_stats is how each test proves that its input reached the case it names.
"""
import ctypes as C

import numpy as np
import pytest

from index_model import ModelError
from keys_model import KeysModel, NONE, TableModel, forge_keys, home, keys_with_low_bits, snapshot_keys
from support import ID_NONE, va, assert_same  # noqa: F401

pytestmark = pytest.mark.gpu

DIM = 8
ERR_INVALID_ARG, ERR_INVALID_VALUE, ERR_UNSUPPORTED, ERR_CORRUPT = 1, 2, 6, 10
CONFIGS = (("f32", "cosine"), ("bf16", "l2"), ("bf16", "ip"))      # all three metrics, both dtypes


def u64(x):
    return np.asarray(x, dtype=np.uint64)


@pytest.fixture(scope="module")
def rows():
    return np.random.default_rng(90210).standard_normal((1200, DIM)).astype(np.float32)


@pytest.fixture(scope="module")
def queries():
    return np.random.default_rng(90211).standard_normal((6, DIM)).astype(np.float32)


def pair(va, raw, dtype="f32", metric="l2", id_offset=0):
    """A handle and its model holding the rows `raw`."""
    m = KeysModel(DIM, dtype, metric, id_offset=id_offset)
    ix = va.Index(DIM, dtype, metric)
    if id_offset:
        ix.set_id_offset(id_offset)
    for h in (ix, m):
        h.add(raw)
    return ix, m


def refused(va, code, call, *a):
    with pytest.raises(va.VrodError) as e:
        call(*a)
    assert e.value.code == code, e.value


def agree(ix, m, probe=(), what=""):
    """The handle reads as the model does: the key column, find over every key either knows plus `probe`, the ids' keys,
    the live keyed count; and the table keeps its load rule."""
    off = m.offset
    assert ix.count == m.count and ix.live_count() == m.live_count(), what
    assert np.array_equal(ix.get_keys(off, m.count), m.get_keys(off, m.count)), what
    pool = np.unique(np.concatenate([m.keys, u64(list(probe)), u64([NONE, 0, 424242])]))
    pool = np.concatenate([pool, pool[:3]])                                      # (repeats)
    assert np.array_equal(ix.find_keys(pool), m.find_keys(pool)), what
    ids = np.concatenate([np.arange(off, off + m.count + 2, dtype=np.uint64), u64([NONE, 0])])
    assert np.array_equal(ix.ids_to_keys(ids), m.ids_to_keys(ids)), what
    st = ix.key_stats()
    assert st["keyed_live"] == m.keyed_live(), (what, st)
    assert st["occupied"] <= st["slots"] // 2 and st["max_probe"] <= max(st["slots"], 1), (what, st)
    assert st["slots"] == 0 or (st["slots"] >= 1024 and st["slots"] & (st["slots"] - 1) == 0), (what, st)
    return st


def test_nothing_before_the_first_set(va, rows):
    ix, m = pair(va, rows[:50])
    with ix:
        assert ix.key_stats() == dict(keyed_live=0, slots=0, occupied=0, rebuilds=0, max_probe=0)
        assert np.array_equal(ix.get_keys(0, 50), np.full(50, ID_NONE))
        assert np.array_equal(ix.find_keys([1, 2, NONE]), np.full(3, ID_NONE))
        assert np.array_equal(ix.ids_to_keys([0, 49, 50, NONE]), np.full(4, ID_NONE))
        assert ix.delete_keys([1, 2]) == 0 and ix.live_count() == 50
        ix.set_keys(0, [])                                                        # n == 0 does nothing
        assert ix.key_stats()["slots"] == 0
        refused(va, ERR_INVALID_ARG, ix.set_keys, 49, [1, 2])                     # a range past the rows
        refused(va, ERR_INVALID_ARG, ix.get_keys, 40, 11)
        assert ix.key_stats()["slots"] == 0
        agree(ix, m)


def test_collisions_and_wrap_around(va, rows):
    ks = keys_with_low_bits(49, 16, 0xFFFF)                                      # one home, the last slot, in every table up to 65536 slots
    assert (home(ks, 1024) == 1023).all() and (home(ks, 65536) == 65535).all()
    ix, m = pair(va, rows[:200])
    with ix:
        for h in (ix, m):
            h.set_keys(100, ks[:48])
        st = agree(ix, m, probe=ks)
        assert st["slots"] == 1024 and st["occupied"] == 48
        assert st["max_probe"] >= 48                                             # 48 keys from the last slot on: the walk wrapped to slot 0
        assert np.array_equal(ix.find_keys(ks[:48]), np.arange(100, 148, dtype=np.uint64))
        assert ix.find_keys(ks[48:])[0] == ID_NONE                               # the same home, 49 slots walked, held by no row


def test_growth_and_rebuild(va, rows):
    ix, m = pair(va, rows[:600])
    t = TableModel()
    with ix:
        for c in range(3):
            keys = np.arange(1000 + 200 * c, 1200 + 200 * c, dtype=np.uint64)
            before = m.keyed_live()
            for h in (ix, m):
                h.set_keys(200 * c, keys)
            t.insert(before, keys, m.holders())
            st = agree(ix, m, what=f"call {c}")
            assert (st["slots"], st["occupied"], st["rebuilds"]) == (t.slots, t.occupied, t.rebuilds), (c, st)
            if c == 0:
                assert st["slots"] == 1024
        assert st["slots"] >= 2048 and st["rebuilds"] >= 1
        for h in (ix, m):
            h.add(rows[600:800])
            h.set_keys(600, np.arange(5000, 5200, dtype=np.uint64))
        st = agree(ix, m)
        assert st["keyed_live"] == 800 and np.array_equal(ix.find_keys(m.keys), np.arange(800, dtype=np.uint64))


def test_stale_slots(va, rows):
    ix, m = pair(va, rows[:300])
    t = TableModel()
    old = []
    with ix:
        rebuilds = []
        for r in range(10):
            keys = np.arange(r * 1000 + 1, r * 1000 + 301, dtype=np.uint64)
            before = m.keyed_live()
            for h in (ix, m):
                h.set_keys(0, keys)
            t.insert(before, keys, keys)
            st = agree(ix, m, probe=old, what=f"round {r}")
            assert st["occupied"] <= st["slots"] // 2
            assert (st["slots"], st["occupied"], st["rebuilds"]) == (t.slots, t.occupied, t.rebuilds), (r, st)
            if old:
                assert (ix.find_keys(old) == ID_NONE).all()
            assert np.array_equal(ix.find_keys(keys), np.arange(300, dtype=np.uint64))
            old.extend(int(k) for k in keys)
            rebuilds.append(st["rebuilds"])
        assert rebuilds[0] == 0 and rebuilds[-1] >= 2 and rebuilds == sorted(rebuilds)


def test_uniqueness(va, rows):
    ix, m = pair(va, rows[:40], id_offset=500)
    with ix:
        for h in (ix, m):
            h.set_keys(500, np.arange(1, 21, dtype=np.uint64))                   # rows 0..19 hold 1..20
            h.delete([505, 506])                                                 # keys 6 and 7 are free; rows 5, 6 store them still

        def both_refuse(first, keys):
            st0, col0, found0 = ix.key_stats(), ix.get_keys(500, 40), ix.find_keys(np.arange(0, 40, dtype=np.uint64))
            refused(va, ERR_INVALID_ARG, ix.set_keys, first, keys)
            with pytest.raises(ModelError):
                m.set_keys(first, keys)
            assert ix.key_stats() == st0 and np.array_equal(ix.get_keys(500, 40), col0)
            assert np.array_equal(ix.find_keys(np.arange(0, 40, dtype=np.uint64)), found0)
            agree(ix, m)

        both_refuse(520, [30, 31, 30])                                           # a key twice within the call
        both_refuse(520, [31, 3])                                                # key 3 is held by live row 2, outside the range
        both_refuse(500, [2, 1, 9])                                              # key 9 is held by row 8, outside [0, 3)
        for first, keys in ((500, [3, 1, 2]),                                    # a permutation inside the range
                            (520, [6]),                                          # held only by a deleted row
                            (504, [77, 78, 78, 79]),                             # rows 4..7: 5 and 6 are deleted, the repeat is between them ...
                            (505, [80, 80]),                                     # ... both deleted
                            (506, [79, 79]),                                     # ... a deleted row (6) and a live one (7)
                            (530, [NONE, NONE]),                                 # no key may repeat
                            (500, [NONE])):                                      # and clears a key
            for h in (ix, m):
                h.set_keys(first, keys)
            agree(ix, m, probe=range(0, 100), what=f"{first} {keys}")
        assert ix.find_keys([3, 1, 2, 6, 79, 80])[0] == ID_NONE                 # row 0 was cleared
        assert np.array_equal(ix.find_keys([1, 2, 6, 79, 80, 78]), u64([501, 502, 520, 507, NONE, NONE]))


def test_delete_frees_a_key(va, rows):
    ix, m = pair(va, rows[:30])
    with ix:
        for h in (ix, m):
            h.set_keys(0, np.arange(100, 130, dtype=np.uint64))
            h.delete([4])
        assert ix.find_keys([104])[0] == ID_NONE and ix.get_keys(4, 1)[0] == 104 and ix.key_stats()["keyed_live"] == 29
        for h in (ix, m):
            h.set_keys(9, [104])                                                 # row 9 gives up 109 for it
        assert np.array_equal(ix.find_keys([104, 109]), u64([9, NONE]))
        agree(ix, m, probe=[109])
        got = ix.delete_keys([100, 100, 999, 104, 109, NONE, 129])               # repeated, unknown, freed, none
        assert got == m.delete_keys([100, 100, 999, 104, 109, NONE, 129]) == 3
        assert ix.live_count() == 26
        agree(ix, m, probe=[100, 104, 129])
        assert ix.delete_keys([]) == 0


@pytest.mark.parametrize("dtype,metric", CONFIGS)
def test_upsert(va, rows, queries, dtype, metric):
    rng = np.random.default_rng(77)
    n0 = 120
    ix, m = pair(va, rows[:n0], dtype, metric, id_offset=10)
    ref = va.Index(DIM, dtype, metric)                                           # gets the equivalent update and add calls
    ref.set_id_offset(10)
    ref.add(rows[:n0])
    labels = rng.integers(0, 5, n0).astype(np.uint32)
    tags = rng.integers(0, 1 << 20, n0).astype(np.uint64)
    values = rng.integers(-50, 50, n0).astype(np.int64)
    keys0 = np.arange(1, n0 + 1, dtype=np.uint64) * np.uint64(7)
    with ix, ref:
        for h in (ix, ref):
            h.set_labels(10, labels)
            h.set_tags(10, tags)
            h.set_values(10, values)
            h.set_keys(10, keys0)
            h.delete([13, 20])
        m.set_keys(10, keys0)
        m.delete([13, 20])
        # held keys (rows 0, 5, 50), new ones, and the key of deleted row 3: free, so it is new as well
        keys = u64([7 * 1, 9001, 7 * 6, 7 * 4, 9002, 7 * 51, 9003])
        new_rows = rows[900:907]
        ids = ix.upsert(keys, new_rows)
        want = m.upsert(keys, new_rows)
        assert np.array_equal(ids, want) and np.array_equal(ids, u64([10, 130, 15, 131, 132, 60, 133]))
        held = np.array([0, 2, 5])
        ref.update(ids[held], new_rows[held])
        fresh = np.array([1, 3, 4, 6])
        ref.add(new_rows[fresh])
        ref.set_keys(130, keys[fresh])
        agree(ix, m, probe=keys)
        n = ix.count
        assert n == ref.count == n0 + 4 and ix.live_count() == ref.live_count()
        assert np.array_equal(ix.get_rows(0, n).view(np.uint32), ref.get_rows(0, n).view(np.uint32))
        assert np.array_equal(ix.get_rows(0, n).view(np.uint32), np.ascontiguousarray(m.prepared()).view(np.uint32))
        assert np.array_equal(ix.get_keys(10, n), ref.get_keys(10, n))
        for get in ("get_labels", "get_tags", "get_values"):                     # updated rows keep theirs, appended rows carry 0
            assert np.array_equal(getattr(ix, get)(10, n), getattr(ref, get)(10, n)), get
        assert np.array_equal(ix.get_labels(10, n0), labels) and not ix.get_labels(10 + n0, 4).any()
        got = ix.search(queries, 10)
        assert_same(*got, *ref.search(queries, 10), "upsert against update + add")
        assert_same(*got, *m.search(queries, 10), "upsert against the model")
        bad = new_rows[:3].copy()
        bad[2, 5] = np.nan
        for keys, raw, code in ((u64([5000, 5001, 5000]), new_rows[:3], ERR_INVALID_ARG),      # a key twice
                                (u64([5000, NONE, 5001]), new_rows[:3], ERR_INVALID_ARG),      # no key
                                (u64([7, 5000, 5001]), bad, ERR_INVALID_VALUE),                # NaN, behind a held key
                                (u64([5000, 5001, 5002]), bad, ERR_INVALID_VALUE)):
            st0 = ix.key_stats()
            refused(va, code, ix.upsert, keys, raw)
            with pytest.raises(ModelError) as e:
                m.upsert(keys, raw)
            assert e.value.code == code
            assert ix.count == n and ix.key_stats() == st0
            assert_same(*ix.search(queries, 10), *got, f"after a refused upsert ({code})")
            agree(ix, m, probe=[5000, 5001, 5002])
        assert ix.upsert([], np.zeros((0, DIM), np.float32)).size == 0


def test_upsert_on_a_handle_without_keys(va, rows, queries):
    ix, m = pair(va, rows[:10], "bf16", "cosine")
    with ix:
        keys = u64([31, 32, 33])
        assert np.array_equal(ix.upsert(keys, rows[20:23]), m.upsert(keys, rows[20:23]))       # all new: the first keys of the handle
        assert np.array_equal(ix.upsert(keys[::-1], rows[30:33]), u64([12, 11, 10]))           # all held
        m.upsert(keys[::-1], rows[30:33])
        st = agree(ix, m)
        assert st["slots"] == 1024 and st["keyed_live"] == 3 and ix.count == 13
        assert_same(*ix.search(queries, 10), *m.search(queries, 10), "search after upserts")


def test_compaction(va, rows, queries):
    ix, m = pair(va, rows[:300], "bf16", "ip", id_offset=1000)
    with ix:
        keys = np.arange(300, dtype=np.uint64) * np.uint64(3) + np.uint64(5)
        dead = u64(np.random.default_rng(3).choice(300, 90, replace=False) + 1000)
        for h in (ix, m):
            h.set_keys(1000, keys)
            h.delete(dead)
        before = ix.key_stats()
        new_ids = ix.compact()
        assert np.array_equal(new_ids, m.compact())
        st = agree(ix, m, probe=keys)
        assert st["rebuilds"] == before["rebuilds"] + 1 and st["occupied"] == st["keyed_live"] == 210 and ix.count == 210
        assert np.array_equal(ix.find_keys(keys), new_ids)                       # the NEW ids; the removed rows' keys answer none
        assert (new_ids[dead.astype(np.int64) - 1000] == ID_NONE).all() and (ix.find_keys(keys) == ID_NONE).sum() == 90
        assert np.array_equal(ix.ids_to_keys(new_ids[new_ids != ID_NONE]), keys[new_ids != ID_NONE])
        for h in (ix, m):                                                        # the freed keys serve again, later rows carry none
            h.add(rows[300:310])
        assert (ix.get_keys(1210, 10) == ID_NONE).all()
        for h in (ix, m):
            h.set_keys(1210, keys[dead.astype(np.int64) - 1000][:10])
        agree(ix, m, probe=keys)
        assert_same(*ix.search(queries, 10), *m.search(queries, 10), "search after compaction")


def test_translate_a_device_result(va, rows, queries):
    import torch
    ix, m = pair(va, rows[:9], "f32", "cosine", id_offset=40)
    with ix:
        for h in (ix, m):
            h.set_keys(40, [11, 12, 13, 14, NONE, 16, 17, 18, 19])
            h.delete([41, 43, 46, 48])                                           # 5 live rows, one of them without a key
        d_ids, _ = ix.search_device(torch.from_numpy(queries[:5]).cuda(), 7)
        ids = d_ids.cpu().numpy().view(np.uint64)
        assert ids.shape == (5, 7) and (ids[:, 5:] == ID_NONE).all() and (ids[:, :5] != ID_NONE).all()
        d_keys = ix.ids_to_keys_device(d_ids)
        keys = d_keys.cpu().numpy().view(np.uint64)
        assert np.array_equal(keys, ix.ids_to_keys(ids)) and np.array_equal(keys, m.ids_to_keys(ids))
        assert (keys[:, 5:] == ID_NONE).all() and (keys[:, :5] == ID_NONE).sum() == 5          # the unkeyed row, once per query
        odd = u64([41, 44, 39, 49, NONE, 40, 48])                                # a deleted row gives the key it stores; not rows: none
        d_odd = torch.from_numpy(odd.view(np.int64)).cuda()
        got = ix.ids_to_keys_device(d_odd).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, u64([12, NONE, NONE, NONE, NONE, 11, 19])) and np.array_equal(got, m.ids_to_keys(odd))


def test_device_forms_equal_host_forms(va, rows):
    import torch
    ix, m = pair(va, rows[:700], id_offset=7)
    with ix:
        keys = np.random.default_rng(8).permutation(5000)[:700].astype(np.uint64)
        for h in (ix, m):
            h.set_keys(7, keys)
            h.delete(np.arange(7, 707, 9, dtype=np.uint64))
        ask = np.concatenate([keys, keys[:50], np.arange(5000, 5300, dtype=np.uint64), u64([NONE, NONE])])   # repeated, unknown, none
        d_ask = torch.from_numpy(ask.view(np.int64)).cuda()
        out = torch.full((ask.size,), 5, dtype=torch.int64, device="cuda")
        got = ix.find_keys_device(d_ask, out_ids=out)
        assert got is out
        got = got.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, ix.find_keys(ask)) and np.array_equal(got, m.find_keys(ask))
        assert (got == ID_NONE).sum() == 78 + 6 + 300 + 2
    with va.Index(DIM, "f32", "l2") as bare:                                     # keys never set: a fill, on the device too
        bare.add(rows[:5])
        assert (bare.find_keys_device(d_ask).cpu().numpy().view(np.uint64) == ID_NONE).all()
        assert (bare.ids_to_keys_device(torch.arange(5, dtype=torch.int64, device="cuda")).cpu().numpy().view(np.uint64) == ID_NONE).all()


@pytest.mark.parametrize("dtype,metric", (("bf16", "cosine"), ("f32", "l2")))
def test_snapshot_round_trip(va, rows, queries, tmp_path, dtype, metric):
    ix, m = pair(va, rows[:330], dtype, metric, id_offset=64)
    a, b = str(tmp_path / "a.vrod"), str(tmp_path / "b.vrod")
    with ix:
        keys = np.arange(330, dtype=np.uint64) + np.uint64(1 << 40)
        for h in (ix, m):
            h.set_keys(64, keys)
            h.delete([70, 71, 200])
            h.set_keys(100, [NONE])
        ix.save(a)
        assert np.array_equal(snapshot_keys(a), m.keys)
        va.snapshot_verify(a)
        with va.Index.load(a) as back:
            assert back.key_stats()["rebuilds"] == 0                             # since the handle was loaded
            st = agree(back, m, probe=keys)
            assert st["keyed_live"] == ix.key_stats()["keyed_live"] == 326 and st["occupied"] == 326
            assert np.array_equal(back.find_keys(keys), ix.find_keys(keys))
            assert_same(*back.search(queries, 10), *ix.search(queries, 10), "search on the loaded handle")
            back.save(b)
            assert open(a, "rb").read() == open(b, "rb").read()                  # save, load, save
            for h in (back, m):                                                  # the loaded table takes inserts like any other
                h.set_keys(70, [5, 6])
                h.set_keys(300, np.arange(30, dtype=np.uint64) + np.uint64(900))
            agree(back, m, probe=keys)


def test_snapshot_never_set_survives(va, rows, tmp_path):
    a, b = str(tmp_path / "a.vrod"), str(tmp_path / "b.vrod")
    with va.Index(DIM, "f32", "l2") as ix:
        ix.add(rows[:40])
        ix.save(a)
        assert snapshot_keys(a) is None                                          # no section: the bytes of a build without keys
        with va.Index.load(a) as back:
            assert back.key_stats() == dict(keyed_live=0, slots=0, occupied=0, rebuilds=0, max_probe=0)
            assert (back.get_keys(0, 40) == ID_NONE).all()
            back.save(b)
        assert open(a, "rb").read() == open(b, "rb").read()


def test_snapshot_with_a_shared_key_is_corrupt(va, rows, tmp_path):
    a, dup, ok = str(tmp_path / "a.vrod"), str(tmp_path / "dup.vrod"), str(tmp_path / "ok.vrod")
    with va.Index(DIM, "bf16", "l2") as ix:
        ix.add(rows[:100])
        ix.set_keys(0, np.arange(1, 101, dtype=np.uint64))
        ix.delete([10])
        ix.save(a)
    keys = snapshot_keys(a)
    forged = keys.copy()
    forged[60] = forged[20]                                                      # two live rows share key 21
    forge_keys(a, dup, forged)
    va.snapshot_verify(dup)                                                      # sound in every respect the file format checks
    refused(va, ERR_CORRUPT, va.Index.load, dup)
    forged = keys.copy()
    forged[10] = forged[20]                                                      # the same repeat, with deleted row 10: allowed
    forge_keys(a, ok, forged)
    with va.Index.load(ok) as back:
        assert back.find_keys([21])[0] == 20 and back.get_keys(10, 1)[0] == 21 and back.key_stats()["keyed_live"] == 99


def test_random_sequence(va, rows, queries):
    rng = np.random.default_rng(4242)
    ix, m = pair(va, rows[:250], "bf16", "l2", id_offset=3)
    fresh = iter(range(10_000, 1_000_000))
    done = {}
    with ix:
        def both(name, *a):
            """The same call on both; refused by both with the same code, or by neither; -> the handle's result."""
            done[name] = done.get(name, 0) + 1
            try:
                want = getattr(m, name)(*a)
            except ModelError as e:
                refused(va, e.code, getattr(ix, name), *a)
                done["refused"] = done.get("refused", 0) + 1
                return None
            got = getattr(ix, name)(*a)
            if want is not None and name != "add":
                assert np.array_equal(got, want), (name, a)
            return got

        def some_keys(n):
            """Held keys, keys held once, fresh keys and, now and then, none."""
            known = m.keys[m.keys != ID_NONE]
            out = []
            for _ in range(n):
                r = rng.random()
                if r < 0.45 and known.size:
                    out.append(int(known[rng.integers(known.size)]))
                elif r < 0.5:
                    out.append(NONE)
                else:
                    out.append(next(fresh) if r < 0.8 else int(rng.integers(1, 400)))
            return u64(out)

        for step in range(400):
            op = rng.choice(["add", "set_keys", "set_keys_fresh", "upsert", "delete", "delete_keys", "update", "compact", "find", "ids_to_keys"],
                            p=[0.06, 0.14, 0.14, 0.16, 0.1, 0.1, 0.08, 0.04, 0.09, 0.09])
            live = np.flatnonzero(~m.deleted)
            if op == "add":
                if m.count < 380:
                    n = int(rng.integers(1, 9))
                    both("add", rows[rng.integers(0, 1200, n)])
            elif op in ("set_keys", "set_keys_fresh"):
                first = int(rng.integers(0, m.count))
                n = int(rng.integers(1, min(40, m.count - first) + 1))
                keys = u64([next(fresh) for _ in range(n)]) if op == "set_keys_fresh" else some_keys(n)
                both("set_keys", first + 3, keys)
            elif op == "upsert":
                keys = some_keys(int(rng.integers(1, 12)))
                if m.count + keys.size < 400:
                    both("upsert", keys, rows[rng.integers(0, 1200, keys.size)])
            elif op == "delete":
                both("delete", u64(rng.integers(0, m.count, int(rng.integers(1, 6))) + 3))
            elif op == "delete_keys":
                keys = some_keys(int(rng.integers(1, 8)))
                assert ix.delete_keys(keys) == m.delete_keys(keys)
                done[op] = done.get(op, 0) + 1
            elif op == "update" and live.size:
                at = rng.choice(live, int(rng.integers(1, 5)))
                both("update", u64(at + 3), rows[rng.integers(0, 1200, at.size)])
            elif op == "compact" and m.live_count() > 150:
                both("compact")
            elif op == "find":
                both("find_keys", some_keys(30))
            elif op == "ids_to_keys":
                both("ids_to_keys", u64(rng.integers(0, m.count + 5, (4, 6)) + 3))
            agree(ix, m, what=f"step {step}: {op}")
            if step % 40 == 39:
                assert_same(*ix.search(queries, 10), *m.search(queries, 10), f"search at step {step}")
        assert_same(*ix.search(queries, 10), *m.search(queries, 10), "search at the end")
        st = ix.key_stats()
        assert st["rebuilds"] >= 1 and done.get("refused", 0) >= 5 and all(done.get(k, 0) >= 5 for k in
                                                                    ("add", "set_keys", "upsert", "delete", "delete_keys", "update", "compact")), (st, done)


def raw_calls(va, ix, torch):
    """Every key entry point through ctypes, outputs pre-filled with 5 -> [(name, status, its output arrays)]."""
    L = va.load()
    n = 4
    keys = u64([1, 2, 3, 4])
    vec = np.zeros((n, DIM), np.float32)
    d_in = torch.from_numpy(keys.view(np.int64)).cuda()
    out = []

    def host(name, call):
        o = np.full(n, 5, np.uint64)
        out.append((name, call(o.ctypes.data_as(C.c_void_p)), o))

    def device(name, fn):
        o = torch.full((n,), 5, dtype=torch.int64, device="cuda")
        rc = fn(ix._h, d_in.data_ptr(), n, o.data_ptr(), None)
        out.append((name, rc, o.cpu().numpy().view(np.uint64)))

    kp, vp_ = keys.ctypes.data_as(C.c_void_p), vec.ctypes.data_as(C.c_void_p)
    host("set_keys", lambda o: L.vrod_index_set_keys(ix._h, 0, kp, n))
    host("find_keys", lambda o: L.vrod_index_find_keys(ix._h, kp, n, o))
    host("ids_to_keys", lambda o: L.vrod_index_ids_to_keys(ix._h, kp, n, o))
    host("upsert", lambda o: L.vrod_index_upsert(ix._h, kp, vp_, n, o))
    died = C.c_uint64(0)
    host("delete_keys", lambda o: L.vrod_index_delete_keys(ix._h, kp, n, C.byref(died)))
    device("find_keys_device", L.vrod_index_find_keys_device)
    device("ids_to_keys_device", L.vrod_index_ids_to_keys_device)
    return out, died.value


def test_unsupported_on_a_multi_device_handle(va, rows):
    import torch
    with va.Index(DIM, "f32", "l2", devices=[0, 0]) as ix:                       # two shards on one device, as the multirank tests make them
        ix.add(rows[:20])
        calls, died = raw_calls(va, ix, torch)
        for name, rc, o in calls:
            assert rc == ERR_UNSUPPORTED and (o == 5).all(), name
        assert died == 0 and ix.count == 20 and ix.live_count() == 20
        assert (ix.get_keys(0, 20) == ID_NONE).all()                             # (get reports what every row carries)
        assert ix.key_stats() == dict(keyed_live=0, slots=0, occupied=0, rebuilds=0, max_probe=0)


def test_refused_while_a_search_is_pending(va, rows, queries):
    import torch
    with va.Index(DIM, "f32", "l2") as ix:
        ix.add(rows[:20])
        ix.set_keys(0, np.arange(1, 21, dtype=np.uint64))
        d_q = torch.from_numpy(queries).cuda()
        d_ids = torch.empty((6, 3), dtype=torch.int64, device="cuda")
        d_sc = torch.empty((6, 3), dtype=torch.float32, device="cuda")
        ix.search_begin_device(d_q, 3, d_ids, d_sc)
        try:
            st0 = ix.key_stats()
            calls, died = raw_calls(va, ix, torch)
            for name, rc, o in calls:
                assert rc == ERR_INVALID_ARG and (o == 5).all(), name
            assert died == 0 and ix.key_stats() == st0
        finally:
            ix.search_end()
        assert ix.count == 20 and ix.live_count() == 20
        assert np.array_equal(ix.find_keys([1, 20, 21]), u64([0, 19, NONE]))
