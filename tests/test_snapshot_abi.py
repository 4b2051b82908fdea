"""CPU tests of the snapshot interface: what needs no device.  The symbols in every layer, the host checksum against
numpy, and files written by snapshot_model.py -- sound ones and each kind of bad one -- through vrod_snapshot_info,
vrod_snapshot_verify and vrod_index_load.  A bad file must fail in vrod_index_load before the device is looked for, so these
tests give the same result on a machine with and without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import snapshot_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vrod_index_save", "vrod_index_load", "vrod_snapshot_info", "vrod_snapshot_verify", "vrod_snapshot_checksum",
       "vrod_snapshot_checksum_device"]
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_IO, ERR_CORRUPT = 1, 6, 9, 10
BYTE_COUNTS = (0, 1, 3, 4, 5, 4095, 4096, 4097)
FIRST_WORDS = (0, 2 ** 32 - 2)                     # the second: word indices straddle 2^32
N, DIM = 70, 3                                     # bf16 rows of odd width: 210 elements, dense words straddle rows


@pytest.fixture(scope="module")
def L():
    import vrod_amd
    return vrod_amd.load()


def make_file(path, full, **over):
    """A sound snapshot of 70 bf16 rows of width 3, with every optional section or with none."""
    rng = np.random.default_rng(7)
    rows = (rng.standard_normal((N, DIM)).astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    deleted = rng.random(N) < 0.2
    a = dict(dim=DIM, dtype=1, metric=1, rows=rows, norms=rng.random(N).astype(np.float32), deleted=deleted, id_offset=2 ** 40 + 5,
             max_xn2_bits=0x40A00000)
    if full:
        a.update(allow=rng.random(N) < 0.5, labels=rng.integers(0, 2 ** 32, N, dtype=np.uint32),
                 tags=rng.integers(0, 2 ** 64, N, dtype=np.uint64), values=rng.integers(-2 ** 63, 2 ** 63, N, dtype=np.int64))
    a.update(over)
    return a, M.write(path, **a)


def info(L, path):
    import vrod_amd._lib as lib
    out = lib.SnapshotInfo()
    rc = L.vrod_snapshot_info(os.fsencode(path), C.byref(out))
    return rc, out.as_dict()


def load(L, path):
    """vrod_index_load -> (status, the handle pointer's value)."""
    h = C.c_void_p(0xDEAD)
    dev = (C.c_int * 1)(0)
    rc = L.vrod_index_load(C.byref(h), os.fsencode(path), dev, 1)
    return rc, h.value


def rejected_everywhere(L, path, code, verify_only=False):
    """`path` is refused with `code` by verify and by load (with *out null) and, unless only the payload is bad, by info."""
    if not verify_only:
        assert info(L, path)[0] == code, L.vrod_last_error()
    assert L.vrod_snapshot_verify(os.fsencode(path)) == code, L.vrod_last_error()
    rc, h = load(L, path)
    assert (rc, h) == (code, None), (rc, h, L.vrod_last_error())


# ---------------------------------------------------------------- symbols
def test_symbols_in_every_layer(L):
    import vrod_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vrod.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", vrod_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for s in NEW:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in vrod_amd.SYMBOLS and getattr(L, s).argtypes is not None, s
        assert re.search(rf"pub fn {s}\s*\(", rust), s
        assert re.search(rf" T {s}\n", exported), s
    assert re.search(r"VROD_ERR_IO = 9\b", hdr) and re.search(r"VROD_ERR_CORRUPT = 10\b", hdr)
    assert (vrod_amd.ERR_IO, vrod_amd.ERR_CORRUPT) == (ERR_IO, ERR_CORRUPT)
    assert callable(vrod_amd.Index.save) and callable(vrod_amd.Index.load)
    assert callable(vrod_amd.snapshot_info) and callable(vrod_amd.snapshot_verify)


# ---------------------------------------------------------------- the checksum
@pytest.mark.parametrize("first_word", FIRST_WORDS)
@pytest.mark.parametrize("n", BYTE_COUNTS)
def test_host_checksum_is_the_numpy_one(L, n, first_word):
    data = np.random.default_rng(n + 1).integers(0, 256, n, dtype=np.uint8)
    out = C.c_uint64(123)
    assert L.vrod_snapshot_checksum(data.ctypes.data_as(C.c_void_p), n, first_word, C.byref(out)) == 0
    assert out.value == M.checksum(data, first_word)
    if n >= 8:      # a sum: two pieces give what the whole gives
        a, b = C.c_uint64(), C.c_uint64()
        L.vrod_snapshot_checksum(data.ctypes.data_as(C.c_void_p), 4, first_word, C.byref(a))
        L.vrod_snapshot_checksum(data[4:].ctypes.data_as(C.c_void_p), n - 4, first_word + 1, C.byref(b))
        assert (a.value + b.value) % 2 ** 64 == out.value


def test_checksum_sees_position_and_fill():
    assert M.checksum(b"") == 0
    assert M.checksum(b"\1") == M.checksum(b"\1\0\0\0") != M.checksum(b"\0\1")
    assert M.checksum(b"\0" * 8) != M.checksum(b"\0" * 4) != 0
    # one word, worked by hand in Python integers
    z = (5 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert M.checksum(b"\5\0\0\0", first_word=2) == z ^ (z >> 31)


# ---------------------------------------------------------------- good files
@pytest.mark.parametrize("full", [True, False], ids=["every-section", "no-optional-section"])
def test_good_file(L, tmp_path, full):
    import vrod_amd
    path = str(tmp_path / "good.vrod")
    a, table = make_file(path, full)
    rc, got = info(L, path)
    assert rc == 0, L.vrod_last_error()
    want = dict(version=1, dim=DIM, dtype=1, metric=1, count=N, live_count=N - int(a["deleted"].sum()), id_offset=2 ** 40 + 5,
                file_bytes=os.path.getsize(path), has_filter=int(full), has_labels=int(full), has_tags=int(full), has_values=int(full))
    assert got == want
    assert vrod_amd.snapshot_info(path) == want
    assert L.vrod_snapshot_verify(os.fsencode(path)) == 0, L.vrod_last_error()
    vrod_amd.snapshot_verify(path)
    assert set(table) == ({1, 2, 3, 4, 5, 6, 7} if full else {1, 2, 3})
    back = M.read(path)                             # the writer and the reader agree with each other
    assert back["max_xn2_bits"] == 0x40A00000 and back["sections"][M.ROWS] == a["rows"].tobytes()


def test_empty_snapshot(L, tmp_path):
    path = str(tmp_path / "empty.vrod")
    M.write(path, dim=8, dtype=0, metric=0, rows=np.zeros((0, 8), np.float32), norms=np.zeros(0, np.float32), deleted=np.zeros(0, bool))
    rc, got = info(L, path)
    assert rc == 0 and got["count"] == 0 and got["file_bytes"] == 4096
    assert L.vrod_snapshot_verify(os.fsencode(path)) == 0


# ---------------------------------------------------------------- bad files
def patched(src, dst, at, new):
    raw = bytearray(open(src, "rb").read())
    raw[at:at + len(new)] = new
    open(dst, "wb").write(bytes(raw))
    return dst


def test_wrong_magic_and_short_header(L, tmp_path):
    good = str(tmp_path / "good.vrod")
    make_file(good, True)
    rejected_everywhere(L, patched(good, str(tmp_path / "magic.vrod"), 0, b"VRODSNAQ"), ERR_CORRUPT)
    raw = open(good, "rb").read()
    for n in (0, 7, 8, 100, 4095):
        short = str(tmp_path / f"short{n}.vrod")
        open(short, "wb").write(raw[:n])
        rejected_everywhere(L, short, ERR_CORRUPT)
    # a header whose own checksum does not hold (a flipped bit in the count)
    rejected_everywhere(L, patched(good, str(tmp_path / "hdr.vrod"), 24, bytes([raw[24] ^ 1])), ERR_CORRUPT)


def test_file_shorter_than_its_table(L, tmp_path):
    good = str(tmp_path / "good.vrod")
    make_file(good, True)
    raw = open(good, "rb").read()
    for cut in (1, 4096, len(raw) - 4096):
        short = str(tmp_path / f"cut{cut}.vrod")
        open(short, "wb").write(raw[:len(raw) - cut])
        rejected_everywhere(L, short, ERR_CORRUPT)
    longer = str(tmp_path / "longer.vrod")
    open(longer, "wb").write(raw + b"\0" * 4096)
    rejected_everywhere(L, longer, ERR_CORRUPT)


@pytest.mark.parametrize("full", [True, False], ids=["every-section", "no-optional-section"])
def test_one_flipped_payload_bit_in_each_section(L, tmp_path, full):
    good = str(tmp_path / "good.vrod")
    _, table = make_file(good, full)
    raw = open(good, "rb").read()
    for kind, (off, nbytes) in table.items():
        for at in (off, off + nbytes - 1):          # the first and the last payload byte (the last: half a word in the rows)
            bad = patched(good, str(tmp_path / f"flip{kind}_{at}.vrod"), at, bytes([raw[at] ^ 0x10]))
            assert info(L, bad)[0] == 0             # the header is sound
            rejected_everywhere(L, bad, ERR_CORRUPT, verify_only=True)


def test_deleted_bits_must_agree_with_the_live_count(L, tmp_path):
    path = str(tmp_path / "live.vrod")
    a, _ = make_file(path, False)
    # a consistent file but for the header's live count (the header's checksum is recomputed)
    back = M.read(path)
    fields = {k: back[k] for k in ("version", "dim", "dtype", "metric", "count", "live_count", "id_offset", "file_bytes", "max_xn2_bits")}
    fields["live_count"] -= 1
    hdr = M.encode_header(fields, [(k, *back["table"][k]) for k in sorted(back["table"])])
    rejected_everywhere(L, patched(path, str(tmp_path / "live_bad.vrod"), 0, hdr), ERR_CORRUPT, verify_only=True)


def test_version_2_and_unknown_sections_are_unsupported(L, tmp_path):
    v2 = str(tmp_path / "v2.vrod")
    make_file(v2, True, version=2)
    rejected_everywhere(L, v2, ERR_UNSUPPORTED)
    good = str(tmp_path / "good.vrod")
    make_file(good, False)
    back = M.read(good)
    fields = {k: back[k] for k in ("version", "dim", "dtype", "metric", "count", "live_count", "id_offset", "file_bytes", "max_xn2_bits")}
    table = [(k, *back["table"][k]) for k in sorted(back["table"])]
    table[2] = (99,) + table[2][1:]                 # a kind this version does not know, in a header that is otherwise sound
    rejected_everywhere(L, patched(good, str(tmp_path / "kind.vrod"), 0, M.encode_header(fields, table)), ERR_UNSUPPORTED)


def test_missing_file_and_directory_are_io_errors(L, tmp_path):
    rejected_everywhere(L, str(tmp_path / "nothing-here.vrod"), ERR_IO)
    assert b"No such file" in L.vrod_last_error()
    rejected_everywhere(L, str(tmp_path), ERR_IO)


def test_more_than_one_device_is_unsupported(L, tmp_path):
    path = str(tmp_path / "good.vrod")
    make_file(path, False)
    h = C.c_void_p(0xDEAD)
    dev = (C.c_int * 2)(0, 0)
    assert L.vrod_index_load(C.byref(h), os.fsencode(path), dev, 2) == ERR_UNSUPPORTED and h.value is None


# ---------------------------------------------------------------- null arguments
def test_null_arguments(L, tmp_path):
    import vrod_amd._lib as lib
    path = os.fsencode(str(tmp_path / "x.vrod"))
    h, out, inf = C.c_void_p(0xDEAD), C.c_uint64(), lib.SnapshotInfo()
    dev = (C.c_int * 1)(0)
    assert L.vrod_index_save(None, path) == ERR_INVALID_ARG
    assert L.vrod_index_save(None, None) == ERR_INVALID_ARG
    assert L.vrod_index_load(None, path, dev, 1) == ERR_INVALID_ARG
    assert L.vrod_index_load(C.byref(h), None, dev, 1) == ERR_INVALID_ARG and h.value is None
    h = C.c_void_p(0xDEAD)
    assert L.vrod_index_load(C.byref(h), path, None, 1) == ERR_INVALID_ARG and h.value is None
    assert L.vrod_snapshot_info(None, C.byref(inf)) == ERR_INVALID_ARG
    assert L.vrod_snapshot_info(path, None) == ERR_INVALID_ARG
    assert L.vrod_snapshot_verify(None) == ERR_INVALID_ARG
    assert L.vrod_snapshot_checksum(None, 4, 0, C.byref(out)) == ERR_INVALID_ARG
    assert L.vrod_snapshot_checksum(C.byref(out), 4, 0, None) == ERR_INVALID_ARG
    assert L.vrod_snapshot_checksum(None, 0, 0, C.byref(out)) == 0 and out.value == 0     # nothing to read: fine
    assert L.vrod_snapshot_checksum_device(0, None, 4, 0, C.byref(out), None) == ERR_INVALID_ARG
    assert L.vrod_snapshot_checksum_device(0, C.c_void_p(4096), 4, 0, None, None) == ERR_INVALID_ARG
    assert L.vrod_last_error()
    assert not os.path.exists(path)
