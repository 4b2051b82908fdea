"""GPU tests of the device-resident ingest: vrod_index_add_device, _update_device, _upsert_device, _get_rows_device.

The host forms prepare their rows with the same kernel, so a second handle fed through them (the twin) is no independent
truth for the stored rows: those are compared with the CPU oracle's prepare of the widened fp32 rows that both handles
were given.  The twin stays the yardstick for everything above the rows: eps_bound and scan_bytes of the stats, a
3-query and a 300-query search (the stream and the batched path, the planes of an fp32 handle included) and the bytes
vrod_index_save writes.  Every comparison is bit for bit."""
import numpy as np
import pytest

from support import ID_NONE, METRIC_COSINE, METRIC_L2, O, THREADS, assert_same_all_bits, bits, oracle_over, special_rows, va  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID_ARG, INVALID_VALUE, UNSUPPORTED = 1, 2, 6
TIMES = ("scan_ms", "total_ms", "sample_ms", "overlap_ms")


def torch_dtype(name):
    import torch
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[name]


def source(rows_f32, src, stride=None, offset=0, fill=0.0):
    """rows (numpy fp32) -> (a CUDA tensor view [n, dim] of dtype `src` whose rows are `stride` elements apart and
    start `offset` elements into their buffer, the same rows widened back to fp32 on the host).  The elements between
    the rows hold `fill`."""
    import torch
    n, dim = rows_f32.shape
    stride = dim if stride is None else stride
    buf = torch.full((offset + n * stride,), fill, dtype=torch_dtype(src), device="cuda")
    view = torch.as_strided(buf, (n, dim), (stride, 1), offset)
    view.copy_(torch.from_numpy(rows_f32).cuda())
    return view, view.float().cpu().numpy()


def queries(nq, dim, seed=99):
    return np.random.default_rng(seed).standard_normal((nq, dim)).astype(np.float32)


def snapshot(ix, path):
    ix.save(str(path))
    return open(path, "rb").read()


def assert_twins(ix, tw, rows, O, tmp_path, what, nqs=(3, 300), k=10):
    """The device-fed handle holds the oracle's prepare of `rows` (the widened fp32 rows both handles were given, row i
    of them in row i of the handles), and the two handles cannot be told apart through the ABI."""
    assert ix.count == tw.count == len(rows) and ix.live_count() == tw.live_count(), what
    n = ix.count
    if n:
        got = bits(ix.get_rows(0, n))
        want = O.prepare(rows, ix.dtype, METRIC_COSINE if ix.metric == METRIC_COSINE else METRIC_L2, threads=THREADS)
        assert np.array_equal(got, bits(want)), f"{what}: get_rows against the oracle"
        assert np.array_equal(got, bits(tw.get_rows(0, n))), f"{what}: get_rows"
    for nq in nqs:
        q = queries(nq, ix.dim)
        kk = min(k, max(1, ix.live_count()))
        i1, s1 = ix.search(q, kk)
        st1 = ix.last_stats()
        i2, s2 = tw.search(q, kk)
        st2 = tw.last_stats()
        assert_same_all_bits(i1, s1, i2, s2, f"{what}: search nq={nq}")
        for key in ("eps_bound", "scan_bytes", "path", "kprime"):
            assert bits(st1[key]).tolist() == bits(st2[key]).tolist() if key == "eps_bound" else st1[key] == st2[key], (what, nq, key, st1, st2)
    assert snapshot(ix, tmp_path / "dev.vrod") == snapshot(tw, tmp_path / "twin.vrod"), f"{what}: snapshot bytes"


def pair(va, dim, dtype, metric, **kw):
    return va.Index(dim, dtype, metric, **kw), va.Index(dim, dtype, metric)


# ---------------------------------------------------------------- add: shapes where the kernel can go wrong
@pytest.mark.parametrize("dim,n", [(1, 70), (3, 70), (63, 70), (64, 70), (65, 70), (768, 300), (769, 70), (32768, 33), (64, 1)])
def test_add_shapes_and_strides(va, O, tmp_path, dim, n):
    """Every row width at which the loads or the work-group shape change (below, at and above a vector, a wave, the
    four-rows-per-group limit), each with row_stride = dim, dim + 1 and dim + 7 (rows on 4- and 2-byte boundaries only)."""
    raw = special_rows(n, dim, dim * 7 + n, "f32")
    for src, dtype, metric in (("f32", "bf16", "cosine"), ("bf16", "f32", "cosine"), ("f16", "bf16", "l2")):
        if dim == 32768 and src != "f32":
            continue                                           # (the wide rows once: they are the slow ones)
        ix, tw = pair(va, dim, dtype, metric)
        with ix, tw:
            for stride, offset in ((dim, 0), (dim + 1, 0), (dim + 7, 1)):
                t, wide = source(raw, src, stride, offset, fill=float("nan"))   # NaN in the padding is never read
                ix.add_device(t)
                tw.add(wide)
            assert_twins(ix, tw, np.concatenate([wide] * 3), O, tmp_path, f"dim {dim} {src}->{dtype}/{metric}",
                         nqs=(3,) if dim == 32768 else (3, 300))


def test_add_column_slice_of_a_wider_tensor(va, O, tmp_path):
    import torch
    dim, n = 96, 500
    for src in ("f32", "bf16", "f16"):
        wide_t = torch.randn((n, 4 * dim + 5), device="cuda").to(torch_dtype(src))
        t = wide_t[:, dim + 3: 2 * dim + 3]                    # stride(0) = 389, the first element at 99
        assert t.stride() == (4 * dim + 5, 1) and not t.is_contiguous()
        ix, tw = pair(va, dim, "bf16", "cosine")
        with ix, tw:
            ix.add_device(t)
            ix.add_device(wide_t[::2, :dim])                   # every second row: stride(0) doubled
            given = [t.float().cpu().numpy(), wide_t[::2, :dim].float().cpu().numpy()]
            for g in given:
                tw.add(g)
            assert_twins(ix, tw, np.concatenate(given), O, tmp_path, f"column slice {src}")


def test_add_crosses_a_staging_chunk(va, tmp_path, O):
    """n = 65536 + 5 at dim 64: two chunks, the second ragged.  This case also goes against the oracle directly."""
    dim, n = 64, 65536 + 5
    raw = special_rows(n, dim, 5, "bf16")
    t, wide = source(raw, "bf16", dim + 1)
    ix, tw = pair(va, dim, "bf16", "cosine")
    with ix, tw:
        ix.add_device(t)
        tw.add(wide)
        assert_twins(ix, tw, wide, O, tmp_path, "two chunks")
        q = queries(7, dim)
        ids, sc = ix.search(q, 10)
        oi, osc = oracle_over(O, wide, q, 10, "bf16", "cosine", np.arange(n))
        assert_same_all_bits(ids, sc, oi, osc, "against the oracle")


# ---------------------------------------------------------------- types
@pytest.mark.parametrize("metric", ["cosine", "l2", "ip"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("src", ["f32", "bf16", "f16"])
def test_types(va, O, tmp_path, src, dtype, metric):
    dim, n = 65, 1000
    raw = special_rows(n, dim, 11, src)
    t, wide = source(raw, src, dim + 3)
    if src == "f16":                                           # the values survived the trip as what they were meant to be
        assert wide[7, 0] == np.float32(1023 * 2.0 ** -24) and wide[5, -1] == np.float32(-(2.0 ** -24)) and wide[6, 0] == 65504.0
    assert np.signbit(wide[4, 0]) and wide[4, 0] == 0.0 and not wide[3].any()
    ix, tw = pair(va, dim, dtype, metric)
    with ix, tw:
        ix.add_device(t)
        tw.add(wide)
        assert_twins(ix, tw, wide, O, tmp_path, f"{src}->{dtype}/{metric}")
        rows = ix.get_rows(0, 8)
        assert not rows[3].any()                               # the zero row stayed zero
        assert np.signbit(rows[4, 0])                          # -0.0 kept its sign


# ---------------------------------------------------------------- refusal
def state_of(ix, q):
    ids, sc = ix.search(q, 5)
    st = ix.last_stats()
    return ix.count, ix.live_count(), bits(ix.get_rows(0, ix.count)).copy(), ids, bits(sc).copy(), bits(st["eps_bound"]).tolist()


def assert_state(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[5] == b[5]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_bad_values_refuse_and_change_nothing(va):
    import torch
    dim, n = 64, 65536 + 5                                     # two chunks
    q = queries(3, dim)
    base = special_rows(500, dim, 3, "f32")
    big, _ = source(special_rows(n, dim, 4, "f32"), "f32", dim + 1, fill=float("nan"))
    with va.Index(dim, "bf16", "cosine") as ix, va.Index(dim, "f32", "l2") as ix2:
        for h in (ix, ix2):
            h.add(base)
        before, before2 = state_of(ix, q), state_of(ix2, q)
        ix.add_device(big)                                     # NaN only in the padding between the rows: accepted
        assert ix.count == 500 + n
    with va.Index(dim, "bf16", "cosine") as ix, va.Index(dim, "f32", "l2") as ix2:
        for h in (ix, ix2):
            h.add(base)
        big[n - 1, dim - 1] = float("nan")                     # the last element of the last row of the second chunk
        for h, was in ((ix, before), (ix2, before2)):
            with pytest.raises(va.VrodError) as e:
                h.add_device(big)
            assert e.value.code == INVALID_VALUE
            assert_state(state_of(h, q), was)
        half = torch.randn((300, dim), device="cuda").to(torch.float16)
        half.view(torch.int16)[150, 31] = 0x7C00               # fp16 +inf, mid-row
        for h, was in ((ix, before), (ix2, before2)):
            with pytest.raises(va.VrodError) as e:
                h.add_device(half)
            assert e.value.code == INVALID_VALUE
            assert_state(state_of(h, q), was)
            h.add_device(half[:150])                           # the rows before it are fine, and the flag was cleared
            assert h.count == 650


# ---------------------------------------------------------------- update
@pytest.mark.parametrize("dtype,metric,src", [("f32", "cosine", "bf16"), ("bf16", "ip", "f16"), ("f32", "l2", "f32")])
def test_update(va, O, tmp_path, dtype, metric, src):
    import torch
    dim, n, m = 65, 3000, 700
    rng = np.random.default_rng(21)
    raw = special_rows(n, dim, 20, "f32")
    ids = rng.permutation(np.setdiff1d(np.arange(n), [17, 18]))[:m].astype(np.int64)   # (17 and 18 are deleted below)
    ids[m // 2] = ids[5]                                       # one id named twice: the last vector wins
    t, wide = source(special_rows(m, dim, 22, src), src, dim + 7, 3)
    d_ids = torch.from_numpy(ids).cuda()
    ix, tw = pair(va, dim, dtype, metric)
    with ix, tw:
        for h in (ix, tw):
            h.add(raw)
            h.delete([17, 18])
            h.search(queries(300, dim), 10)                    # a batched search: an fp32 handle has its planes now
        ix.update_device(d_ids, t)
        tw.update(ids, wide)
        now = raw.copy()
        now[ids] = wide                                        # (numpy too lets the last of two assignments to a row win)
        assert np.array_equal(now[ids[5]], wide[m // 2])
        assert_twins(ix, tw, now, O, tmp_path, f"update {src}->{dtype}/{metric}")
        q = queries(3, dim)
        was = state_of(ix, q)
        for bad in (17, n, 2 ** 40):                           # a deleted row, out of range
            bad_ids = d_ids.clone()
            bad_ids[m - 1] = bad
            with pytest.raises(va.VrodError) as e:
                ix.update_device(bad_ids, t)
            assert e.value.code == INVALID_ARG
            assert_state(state_of(ix, q), was)


def test_update_of_several_chunks_checks_every_row_first(va, O, tmp_path):
    import torch
    dim, n = 64, 65536 + 5
    raw = special_rows(n, dim, 30, "f32")
    t, wide = source(special_rows(n, dim, 31, "bf16"), "bf16", dim + 1)
    d_ids = torch.arange(n - 1, -1, -1, dtype=torch.int64, device="cuda")
    q = queries(3, dim)
    ix, tw = pair(va, dim, "bf16", "cosine")
    with ix, tw:
        ix.add(raw)
        tw.add(raw)
        was = state_of(ix, q)
        t[n - 2, 7] = float("nan")                             # in the last chunk
        with pytest.raises(va.VrodError) as e:
            ix.update_device(d_ids, t)
        assert e.value.code == INVALID_VALUE
        assert_state(state_of(ix, q), was)
        t[n - 2, 7] = 0.5
        wide[n - 2, 7] = 0.5
        ix.update_device(d_ids, t)
        tw.update(d_ids.cpu().numpy(), wide)
        assert_twins(ix, tw, wide[::-1], O, tmp_path, "update over two chunks", nqs=(3,))


# ---------------------------------------------------------------- upsert
def key_state(ix):
    """The key stats that two handles with the same history share.  max_probe is left out: the keys of one call are
    inserted by concurrent threads, and the longest walk depends on which of two keys that meet claims a slot first
    (two runs of the HOST form differ in it too); it is only bounded, as tests/test_gpu_keys.py bounds it."""
    st = ix.key_stats()
    assert 0 <= st.pop("max_probe") <= max(st["slots"], 1)
    return st


def test_upsert(va, O, tmp_path):
    import torch
    dim, n, m = 65, 2000, 600
    raw = special_rows(n, dim, 40, "f32")
    keys0 = (np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(13))
    rng = np.random.default_rng(41)
    held = rng.permutation(n)[: m // 2]
    keys = np.empty(m, np.uint64)
    keys[0::2] = keys0[held]                                   # held and new keys interleaved in one call
    keys[1::2] = np.arange(m // 2, dtype=np.uint64) + np.uint64(1 << 50)
    t, wide = source(special_rows(m, dim, 42, "f16"), "f16", dim + 1, 1)
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    q = queries(3, dim)
    ix, tw = pair(va, dim, "bf16", "cosine")
    with ix, tw:
        for h in (ix, tw):
            h.add(raw)
            h.set_keys(0, keys0)
            h.delete([int(held[0])])                           # its key is free: the upsert appends a row for it
        got = ix.upsert_device(d_keys, t)
        want = tw.upsert(keys, wide)
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
        assert key_state(ix) == key_state(tw)
        assert np.array_equal(ix.get_keys(0, ix.count), tw.get_keys(0, tw.count))
        now = np.concatenate([raw, np.zeros((int((want >= n).sum()), dim), np.float32)])
        now[want.astype(np.int64)] = wide                      # the call's row i lies in row want[i], held or appended
        assert_twins(ix, tw, now, O, tmp_path, "upsert")
        was, kst = state_of(ix, q), key_state(ix)
        for bad in (int(keys[0]), int(ID_NONE)):               # a key twice, VROD_ID_NONE as a key
            bad_keys = keys.copy()
            bad_keys[m - 1] = bad
            with pytest.raises(va.VrodError) as e:
                ix.upsert_device(torch.from_numpy(bad_keys.view(np.int64)).cuda(), t)
            assert e.value.code == INVALID_ARG
            assert_state(state_of(ix, q), was)
            assert key_state(ix) == kst
        t[m - 1, 0] = float("inf")
        with pytest.raises(va.VrodError) as e:
            ix.upsert_device(d_keys, t)
        assert e.value.code == INVALID_VALUE
        assert_state(state_of(ix, q), was)
        assert key_state(ix) == kst and np.array_equal(ix.get_keys(0, ix.count), tw.get_keys(0, tw.count))


# ---------------------------------------------------------------- get_rows_device
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_get_rows_device(va, dtype):
    import torch
    dim, n = 65, 400
    with va.Index(dim, dtype, "cosine") as ix:
        ix.add(special_rows(n, dim, 50, "f32"))
        want = ix.get_rows(37, 300)
        assert np.array_equal(bits(ix.get_rows_device(37, 300).cpu().numpy()), bits(want))
        buf = torch.full((300, dim + 3), -7.25, device="cuda")
        out = ix.get_rows_device(37, 300, out=buf[:, :dim])
        assert out.data_ptr() == buf.data_ptr()
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[:, :dim]), bits(want)) and (got[:, dim:] == -7.25).all()   # the padding is untouched
        with pytest.raises(va.VrodError) as e:
            ix.get_rows_device(101, 300)
        assert e.value.code == INVALID_ARG


# ---------------------------------------------------------------- stream
def test_source_produced_on_a_side_stream(va, O, tmp_path):
    import torch
    dim, n = 768, 4000
    side = torch.cuda.Stream()
    a = torch.randn((n, dim), device="cuda")
    torch.cuda.synchronize()
    ix, tw = pair(va, dim, "bf16", "cosine")
    with ix, tw:
        with torch.cuda.stream(side):                          # the producer runs on `side`, which the call is handed
            t = a
            for _ in range(20):
                t = t @ torch.eye(dim, device="cuda") * 1.0009765625
            t = t.to(torch.bfloat16)
            ix.add_device(t)
        side.synchronize()
        given = t.float().cpu().numpy()
        tw.add(given)
        assert_twins(ix, tw, given, O, tmp_path, "side stream", nqs=(3,))


# ---------------------------------------------------------------- multi-device rehearsal
@pytest.mark.parametrize("staged", [False, True])
def test_two_shards_on_one_device(va, monkeypatch, staged):
    """devices=[0, 0]: add_device and update_device across the shard boundary give a single-device twin's search bits.
    staged: VROD_INGEST_STAGE=1 sends every source the way of one on another device (packed, copied peer to peer)."""
    import torch
    if staged:
        monkeypatch.setenv("VROD_INGEST_STAGE", "1")
    dim, n = 64, 65536 + 700
    t, wide = source(special_rows(n, dim, 60, "bf16"), "bf16", dim + 1)
    rng = np.random.default_rng(61)
    ids = np.concatenate([rng.integers(0, 65536, 300), rng.integers(65536, n, 300)]).astype(np.int64)
    rng.shuffle(ids)
    ids[10] = ids[400]
    u, uwide = source(special_rows(600, dim, 62, "f16"), "f16", dim + 7)
    ix, tw = pair(va, dim, "bf16", "cosine", devices=[0, 0])
    with ix, tw:
        ix.add_device(t[:1000])                                # then across the boundary at row 65536
        ix.add_device(t[1000:])
        tw.add(wide)
        ix.update_device(torch.from_numpy(ids).cuda(), u)
        tw.update(ids, uwide)
        assert ix.count == tw.count == n
        for nq in (3, 300):
            q = queries(nq, dim)
            i1, s1 = ix.search(q, 10)
            i2, s2 = tw.search(q, 10)
            assert_same_all_bits(i1, s1, i2, s2, f"two shards nq={nq}")
        assert np.array_equal(bits(ix.get_rows_device(65000, 1200).cpu().numpy()), bits(tw.get_rows(65000, 1200)))
        buf = torch.full((1200, dim + 3), -7.25, device="cuda")
        ix.get_rows_device(65000, 1200, out=buf[:, :dim])
        assert np.array_equal(bits(buf[:, :dim].cpu().numpy()), bits(tw.get_rows(65000, 1200))) and (buf[:, dim:] == -7.25).all()
        # a bad value in a later shard's rows: no shard keeps a row of the call
        q = queries(3, dim)
        was = (ix.count, ix.search(q, 5))
        u[599, 3] = float("nan")
        with pytest.raises(va.VrodError) as e:
            ix.update_device(torch.from_numpy(ids).cuda(), u)
        assert e.value.code == INVALID_VALUE
        now = ix.search(q, 5)
        assert ix.count == was[0] and np.array_equal(now[0], was[1][0]) and np.array_equal(bits(now[1]), bits(was[1][1]))
        keys = torch.arange(600, dtype=torch.int64, device="cuda")
        with pytest.raises(va.VrodError) as e:
            ix.upsert_device(keys, u)
        assert e.value.code == UNSUPPORTED and ix.count == n


# ---------------------------------------------------------------- pending search
def test_refused_while_a_search_is_pending(va, O):
    import torch
    dim, n, k = 64, 5000, 10
    raw = special_rows(n, dim, 70, "f32")
    q = queries(3, dim)
    t, _ = source(special_rows(10, dim, 71, "bf16"), "bf16")
    d10 = torch.arange(10, dtype=torch.int64, device="cuda")
    with va.Index(dim, "bf16", "cosine") as ix:
        ix.add(raw)
        ix.set_keys(0, np.arange(n, dtype=np.uint64))
        dq = torch.from_numpy(q).cuda()
        oi = torch.empty((3, k), dtype=torch.int64, device="cuda")
        osc = torch.empty((3, k), dtype=torch.float32, device="cuda")
        ix.search_begin_device(dq, k, oi, osc)
        for call in (lambda: ix.add_device(t), lambda: ix.update_device(d10, t), lambda: ix.upsert_device(d10, t),
                     lambda: ix.get_rows_device(0, 10)):
            with pytest.raises(va.VrodError) as e:
                call()
            assert e.value.code == INVALID_ARG and "pending" in str(e.value) and ix.pending == 1
        ix.search_end()
        want_i, want_s = oracle_over(O, raw, q, k, "bf16", "cosine", np.arange(n))
        assert_same_all_bits(oi.cpu().numpy().view(np.uint64), osc.cpu().numpy(), want_i, want_s, "the pending search")
        assert ix.count == n
