"""Index snapshots on the device: vrod_index_save / vrod_index_load.

The files the library writes are read back with the numpy reader of snapshot_model.py (the pin of the format) and compared
byte for byte with what the handle reports; a handle loaded in the middle of a sequence_plans.py plan takes the place of
the one that was saved and must go on matching index_model.ModelIndex in every search form, bit for bit.  The chunk
override puts the seams of the row stream (several chunks, a ragged last one, dense words that straddle rows) at sizes a
test can afford."""
import ctypes as C
import os

import numpy as np
import pytest

import sequence_plans as S
import snapshot_model as M
from conftest import f32_split
from sequence_exec import Pair, same_lists
from support import PATH_AUTO, PATH_EXACT, assert_same, bits

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_IO, ERR_CORRUPT = 1, 6, 9, 10
BYTE_COUNTS = (0, 1, 3, 4, 5, 4095, 4096, 4097, (1 << 20) + 3)
FIRST_WORDS = (0, 2 ** 32 - 2)
TIMES = ("scan_ms", "total_ms", "sample_ms", "overlap_ms")


@pytest.fixture(scope="module")
def va(oracle):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a device"
    import vrod_amd
    vrod_amd.load()
    return vrod_amd


@pytest.fixture
def chunk32(monkeypatch):
    monkeypatch.setenv("VROD_DEBUG_SNAPSHOT_CHUNK_ROWS", "32")


def rows(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


# ---------------------------------------------------------------- the checksum kernel
@pytest.mark.parametrize("first_word", FIRST_WORDS)
def test_device_checksum_is_the_host_one(va, first_word):
    import torch
    L = va.load()
    rng = np.random.default_rng(3)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in BYTE_COUNTS:
        for shift in (0, 4):                        # a 16-byte aligned address, and one that is only 4-byte aligned
            host = rng.integers(0, 256, n + shift, dtype=np.uint8)
            dev = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            got, want = C.c_uint64(1), C.c_uint64(2)
            assert L.vrod_snapshot_checksum_device(0, C.c_void_p(dev.data_ptr() + shift if n else 0), n, first_word, C.byref(got), stream) == 0, \
                L.vrod_last_error()
            assert L.vrod_snapshot_checksum(host[shift:].ctypes.data_as(C.c_void_p), n, first_word, C.byref(want)) == 0
            assert got.value == want.value == M.checksum(host[shift:], first_word), (n, shift, first_word)
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert L.vrod_snapshot_checksum_device(0, C.c_void_p(dev.data_ptr() + 2), 8, 0, C.byref(got), stream) == ERR_INVALID_ARG


# ---------------------------------------------------------------- round trip by sections
def build(va, rng, dtype, metric, dim, count, state):
    """A handle of `count` rows and what its side arrays hold.  state: "none" (nothing ever set), "some" (labels and
    values, rows deleted; no filter, no tags) or "all"."""
    ix = va.Index(dim, dtype, metric)
    ix.set_id_offset(7_000_000_000)
    want = dict(deleted=np.zeros(count, bool), allow=None, labels=None, tags=None, values=None)
    if count:
        ix.add(rows(rng, count, dim))
    if state != "none" and count:
        dead = rng.choice(count, max(1, count // 7), replace=False)
        ix.delete(dead.astype(np.uint64) + np.uint64(7_000_000_000))
        want["deleted"][dead] = True
        want["labels"] = rng.integers(0, 2 ** 32, count, dtype=np.uint32)
        ix.set_labels(7_000_000_000, want["labels"])
        want["values"] = rng.integers(-2 ** 63, 2 ** 63, count, dtype=np.int64)
        ix.set_values(7_000_000_000, want["values"])
        if state == "all":
            want["tags"] = rng.integers(0, 2 ** 64, count, dtype=np.uint64)
            ix.set_tags(7_000_000_000, want["tags"])
            n_rows = count - count // 5             # a filter over fewer rows than the handle has: the rest is not allowed
            allow = rng.random(n_rows) < 0.6
            ix.set_filter(allow)
            want["allow"] = np.concatenate([allow, np.zeros(count - n_rows, bool)])
    return ix, want


def check_file(path, ix, want, dtype, metric, dim, count):
    snap = M.read(path)                             # every checksum, offset, size and padding byte is checked in there
    assert (snap["dim"], snap["dtype"], snap["metric"]) == (dim, {"f32": 0, "bf16": 1}[dtype], {"cosine": 0, "l2": 1, "ip": 2}[metric])
    assert (snap["count"], snap["live_count"], snap["id_offset"]) == (count, ix.live_count(), 7_000_000_000)
    stored = ix.get_rows(0, count) if count else np.zeros((0, dim), np.float32)
    dense = M.to_bf16_bits(stored).tobytes() if dtype == "bf16" else np.ascontiguousarray(stored, "<f4").tobytes()
    sec = snap["sections"]
    assert sec[M.ROWS] == dense, "the row section is not the handle's rows, dense"
    norms = np.frombuffer(sec[M.NORMS], "<f4")
    np.testing.assert_allclose(norms, (stored.astype(np.float64) ** 2).sum(axis=1), rtol=1e-5, atol=1e-30)
    assert snap["max_xn2_bits"] == (int(norms.max().view(np.uint32)) if count else 0)
    assert sec[M.DELETED] == M.pack_bits(want["deleted"]).tobytes()
    for name, kind, dt in (("allow", M.FILTER, None), ("labels", M.LABELS, "<u4"), ("tags", M.TAGS, "<u8"), ("values", M.VALUES, "<i8")):
        if want[name] is None:
            assert kind not in sec, f"a {name} section in the file of a handle that never set one"
        else:
            assert sec[kind] == (M.pack_bits(want[name]).tobytes() if dt is None else np.ascontiguousarray(want[name], dt).tobytes()), name
    return snap


@pytest.mark.parametrize("dim", [1, 3, 64, 770])
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_round_trip_by_sections(va, tmp_path, chunk32, dtype, metric, dim):
    rng = np.random.default_rng(dim * 10 + len(metric))
    for count, state in ((0, "none"), (1, "none"), (33, "all"), (1000, "some")):
        a, b, c = (str(tmp_path / f"{count}{x}.vrod") for x in "abc")
        ix, want = build(va, rng, dtype, metric, dim, count, state)
        with ix:
            ix.save(a)
            snap = check_file(a, ix, want, dtype, metric, dim, count)
            ix.save(b)
            assert open(b, "rb").read() == snap["raw"], "a second save of the same handle differs"
            with va.Index.load(a) as ld:
                assert (ld.dim, ld.dtype, ld.metric) == (ix.dim, ix.dtype, ix.metric)
                assert (ld.count, ld.live_count(), ld.filter_count()) == (ix.count, ix.live_count(), ix.filter_count())
                if count:
                    assert np.array_equal(bits(ld.get_rows(0, count)), bits(ix.get_rows(0, count)))
                    first = 7_000_000_000
                    assert np.array_equal(ld.get_labels(first, count), ix.get_labels(first, count))
                    assert np.array_equal(ld.get_tags(first, count), ix.get_tags(first, count))
                    assert np.array_equal(ld.get_values(first, count), ix.get_values(first, count))
                    q = rows(rng, 5, dim)
                    assert_same(*ld.search(q, 4), *ix.search(q, 4), f"{count} rows")
                ld.save(c)
            assert open(c, "rb").read() == snap["raw"], "save, load, save differs"
        assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]


def test_default_chunks_give_the_same_file(va, tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    with va.Index(100, "bf16", "l2") as ix:
        ix.add(rows(rng, 3000, 100))
        ix.save(str(tmp_path / "default.vrod"))
        for chunk in ("32", "1024", "999999999"):
            monkeypatch.setenv("VROD_DEBUG_SNAPSHOT_CHUNK_ROWS", chunk)
            ix.save(str(tmp_path / "chunked.vrod"))
            assert open(tmp_path / "chunked.vrod", "rb").read() == open(tmp_path / "default.vrod", "rb").read(), chunk
            with va.Index.load(str(tmp_path / "default.vrod")) as ld:
                assert np.array_equal(bits(ld.get_rows(0, 3000)), bits(ix.get_rows(0, 3000))), chunk


# ---------------------------------------------------------------- a loaded handle against the model
SMALL = (
    (18, S.Config("bf16-cosine-100-small", 100, "bf16", "cosine", small=True)),
    (19, S.Config("f32-ip-64-default-small", 64, "f32", "ip", split=None, small=True)),
    (20, S.Config("bf16-l2-33-small", 33, "bf16", "l2", small=True)),
    (21, S.Config("f32-l2-72-split1-offset-small", 72, "f32", "l2", split="1", id_offset=2 ** 40 + 5, small=True)),
)


def tagged_results(ix, rng_seed, dim, live):
    """Tags and values are not part of the model: the searches that read them, for comparison between two handles."""
    rng = np.random.default_rng(rng_seed)
    q = rows(rng, 6, dim)
    preds = np.zeros(6, ix_where_dtype())
    preds["any"], preds["lo"], preds["hi"] = [1, 2, 4, 0, 3, 8], -50, 50
    tp = np.stack([preds["any"], preds["all"], preds["none"]], axis=1)
    return ix.search_tagged(q, 5, tp), ix.search_where(q, 5, preds)


def ix_where_dtype():
    import vrod_amd
    return vrod_amd.WHERE_DTYPE


def swap_for_loaded(p, va, path, what):
    """Save the pair's handle, load the file, destroy the original and go on with the loaded handle."""
    m = p.model
    tag_rng = np.random.default_rng(p.seed)
    tags = tag_rng.integers(0, 16, m.count, dtype=np.uint64)
    values = tag_rng.integers(-100, 100, m.count, dtype=np.int64)
    p.ix.set_tags(m.offset, tags)
    p.ix.set_values(m.offset, values)
    before = tagged_results(p.ix, p.seed, p.cfg.dim, m.live_count())
    p.ix.save(path)
    p.ix.close()
    with f32_split(p.cfg.split):
        p.ix = va.Index.load(path)
    p.state(f"{what}: the loaded handle")
    assert np.array_equal(p.ix.get_tags(m.offset, m.count), tags) and np.array_equal(p.ix.get_values(m.offset, m.count), values)
    after = tagged_results(p.ix, p.seed, p.cfg.dim, m.live_count())
    for g, w in zip(after, before):
        same_lists(g, w, f"{what}: tagged / where search")
    p.read_back(np.arange(m.count), f"{what}: every row, live or deleted")


@pytest.mark.parametrize("seed,cfg", SMALL, ids=[cfg.name for _, cfg in SMALL])
def test_loaded_handle_continues_the_plan(va, tmp_path, chunk32, seed, cfg):
    plan = S.make_plan(seed, cfg)
    kinds = [op.kind for op in plan]
    cut = kinds.index("compact") - 1                # deletes, a filter, labels and updates behind it, the compaction ahead
    assert {"add", "delete", "set_filter", "set_labels", "update"} <= set(kinds[:cut]) and "add" in kinds[cut:]
    with Pair(va, cfg, seed) as p:
        path = PATH_AUTO
        for p.step, op in enumerate(plan):
            if p.step == cut:
                swap_for_loaded(p, va, str(tmp_path / "mid.vrod"), f"before step {cut}")
                p.ix.set_path(path)                 # (vrod_index_set_path is not part of a snapshot)
                p.check_every_form("right after the load", nqs=(3, 40))
            if op.kind == "set_path":
                path = op.a["path"]
            if op.kind == "reject":
                p.reject(op)
            elif S.is_check(op):
                p.check(op)
            else:
                p.mutate(op)
        p.check_every_form("at the end of the plan", nqs=(9,))
        swap_for_loaded(p, va, str(tmp_path / "end.vrod"), "at the end")       # after a compaction and under a narrow filter
        p.check_every_form("the second loaded handle", nqs=(9,))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_eps_bound_follows_the_saved_maximum(va, tmp_path, dtype):
    """The row with the largest norm is updated away: the bound still follows the largest norm the handle has ever held
    (include/vrod.h, vrod_index_update), and the loaded handle must report that bound, not a fresh handle's."""
    rng = np.random.default_rng(9)
    n, d = 3000, 64
    raw = rows(rng, n, d)
    raw[17] *= 40.0
    q = rows(rng, 40, d)
    with va.Index(d, dtype, "l2") as ix:
        ix.add(raw)
        small = rows(rng, 1, d)
        ix.update([17], small)
        ids, sc = ix.search(q, 10)
        st = ix.last_stats()
        assert st["path"] != PATH_EXACT and np.isfinite(st["eps_bound"]) and st["eps_bound"] > 0, st
        ix.save(str(tmp_path / "eps.vrod"))
    with va.Index.load(str(tmp_path / "eps.vrod")) as ld:
        assert_same(*ld.search(q, 10), ids, sc, "the loaded handle")
        st2 = ld.last_stats()
    assert np.float32(st2["eps_bound"]).view(np.uint32) == np.float32(st["eps_bound"]).view(np.uint32), (st, st2)
    for key in ("path", "scan_bytes", "scan_flops", "kprime"):
        assert st2[key] == st[key], (key, st, st2)
    raw[17] = small[0]
    with va.Index(d, dtype, "l2") as fresh:         # the carried scalar matters: without it the bound would be this one
        fresh.add(raw)
        fresh.search(q, 10)
        assert fresh.last_stats()["eps_bound"] < st["eps_bound"]


# ---------------------------------------------------------------- save leaves the handle alone
def test_save_leaves_the_handle_alone(va, tmp_path, chunk32):
    import torch
    rng = np.random.default_rng(11)
    n, d = 2500, 72
    with va.Index(d, "bf16", "cosine") as ix:
        ix.add(rows(rng, n, d))
        ix.delete(rng.choice(n, 100, replace=False).astype(np.uint64))
        ix.set_filter(rng.random(n) < 0.7)
        ix.set_labels(0, rng.integers(0, 5, n, dtype=np.uint32))
        q = rows(rng, 40, d)

        def probe():
            out = []
            for path in (va.PATH_AUTO, va.PATH_STREAM, va.PATH_MFMA, va.PATH_GATHER):
                ix.set_path(path)
                ids, sc = ix.search(q[:3] if path == va.PATH_STREAM else q, 10)
                st = {k: v for k, v in ix.last_stats().items() if k not in TIMES}
                out.append((ids, sc, st))
            ix.set_path(va.PATH_AUTO)
            ids, sc, _ = ix.search_grouped(q[:5], 3)
            out.append((ids, sc, {k: v for k, v in ix.last_stats().items() if k not in TIMES}))
            return out

        probe()                                     # (warm: the self-tuned margin has taken its first steps)
        first = probe()
        ix.save(str(tmp_path / "a.vrod"))
        for (i1, s1, st1), (i2, s2, st2) in zip(first, probe()):
            assert_same(i2, s2, i1, s1, "a search repeated around a save")
            assert st1 == st2, (st1, st2)
        # a pipelined chain whose graph was captured before the save is replayed after it
        dq = [torch.from_numpy(q[:3].copy()).cuda() for _ in range(2)]
        out = [(torch.empty((3, 10), dtype=torch.int64, device="cuda"), torch.empty((3, 10), dtype=torch.float32, device="cuda")) for _ in range(2)]
        ix.set_path(va.PATH_STREAM)

        def chain():
            res = []
            ix.search_begin_device(dq[0], 10, *out[0])
            for s in range(6):
                if s + 1 < 6:
                    ix.search_begin_device(dq[(s + 1) % 2], 10, *out[(s + 1) % 2])
                ix.search_end()
                res.append((out[s % 2][0].cpu().numpy().copy(), out[s % 2][1].cpu().numpy().copy()))
            return res, {k: v for k, v in ix.last_stats().items() if k not in TIMES}
        c1, st1 = chain()
        ix.save(str(tmp_path / "b.vrod"))
        c2, st2 = chain()
        assert st1 == st2
        for (i1, s1), (i2, s2) in zip(c1, c2):
            assert np.array_equal(i1, i2) and np.array_equal(bits(s1), bits(s2))
        # with a search pending a save is refused and writes nothing
        ix.search_begin_device(dq[0], 10, *out[0])
        with pytest.raises(va.VrodError) as e:
            ix.save(str(tmp_path / "pending.vrod"))
        assert e.value.code == ERR_INVALID_ARG and ix.pending == 1
        ix.search_end()
        assert sorted(os.listdir(tmp_path)) == ["a.vrod", "b.vrod"]
        assert open(tmp_path / "a.vrod", "rb").read() == open(tmp_path / "b.vrod", "rb").read()


# ---------------------------------------------------------------- failure behaviour
def test_failures(va, tmp_path):
    rng = np.random.default_rng(13)
    n, d = 1000, 770                                # 3 MB of fp32 rows: past the size the host checks before the device
    good, other = str(tmp_path / "good.vrod"), str(tmp_path / "other.vrod")
    with va.Index(d, "f32", "ip") as ix:
        ix.add(rows(rng, n, d))
        with pytest.raises(va.VrodError) as e:
            ix.save(str(tmp_path / "no-such-dir" / "x.vrod"))
        assert e.value.code == ERR_IO and os.listdir(tmp_path) == []
        ix.save(good)
        ix.delete([5])
        open(other, "wb").write(open(good, "rb").read())
        ix.save(other)                              # over an existing snapshot
        assert sorted(os.listdir(tmp_path)) == ["good.vrod", "other.vrod"]
        assert va.snapshot_info(other)["live_count"] == n - 1 and va.snapshot_info(good)["live_count"] == n
        want = ix.get_rows(0, n)
    va.snapshot_verify(good)
    snap = M.read(good)
    off, nbytes, _ = snap["table"][M.ROWS]
    assert nbytes > 1 << 20
    L = va.load()
    dev = (C.c_int * 1)(0)
    for at in (off, off + nbytes // 2 + 1, off + nbytes - 1):
        raw = bytearray(snap["raw"])
        raw[at] ^= 0x04
        bad = str(tmp_path / "bad.vrod")
        open(bad, "wb").write(bytes(raw))
        h = C.c_void_p(0xDEAD)
        assert L.vrod_index_load(C.byref(h), os.fsencode(bad), dev, 1) == ERR_CORRUPT and h.value is None
        assert b"device memory" in L.vrod_last_error()
    with va.Index.load(good) as ld:                 # a good load on the same device afterwards
        assert ld.count == n and ld.live_count() == n
        assert np.array_equal(bits(ld.get_rows(0, n)), bits(want))
    with va.Index(d, "f32", "ip", devices=[0, 0]) as two:
        two.add(rows(rng, 10, d))
        with pytest.raises(va.VrodError) as e:
            two.save(str(tmp_path / "two.vrod"))
        assert e.value.code == ERR_UNSUPPORTED and not os.path.exists(tmp_path / "two.vrod") and not os.path.exists(tmp_path / "two.vrod.tmp")
