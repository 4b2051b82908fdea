"""The snapshot file format (DESIGN.md "Snapshots", version 1) restated in numpy: the checksum, a writer and a reader.

Independent of the C code: tests/test_snapshot_abi.py feeds files written here to the library, tests/test_gpu_snapshot.py
reads the library's files back with the reader.  Nothing here imports the library.

Layout, little-endian: a 4096-byte header -- "VRODSNAP", u32 version, dim, dtype, metric, u64 count, live_count, id_offset,
file_bytes, u32 max_xn2_bits, n_sections, then at byte 64 n_sections x (u32 kind, u32 0, u64 offset, u64 bytes, u64
checksum), and in its last 8 bytes the checksum of the 4088 before -- followed by the sections, each on a 4096-byte
boundary, zero-padded.
"""
import numpy as np

BLOCK = 4096
MAGIC = b"VRODSNAP"
VERSION = 1
ROWS, NORMS, DELETED, FILTER, LABELS, TAGS, VALUES = 1, 2, 3, 4, 5, 6, 7
OPTIONAL = {"filter": FILTER, "labels": LABELS, "tags": TAGS, "values": VALUES}
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
TABLE_AT, ENTRY, SUM_AT = 64, 32, 4088


def checksum(data, first_word=0) -> int:
    """The section checksum of `data` (bytes, or an array whose bytes are meant): the sum mod 2^64 over the little-endian
    u32 words w_i, the last one zero-filled, of mix(w_i + (first_word + i + 1) * golden)."""
    b = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
    b += b"\0" * (-len(b) % 4)
    w = np.frombuffer(b, dtype="<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        i = np.uint64(first_word % 2 ** 64) + np.arange(w.size, dtype=np.uint64) + np.uint64(1)
        z = w + i * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        z ^= z >> np.uint64(31)
        return int(z.sum(dtype=np.uint64))


def to_bf16_bits(x) -> np.ndarray:
    """fp32 values that are exactly bf16 (what get_rows returns on a BF16 handle) -> their 16 stored bits."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any(), "not bf16 values"
    return (u >> np.uint32(16)).astype("<u2")


def pack_bits(flags) -> np.ndarray:
    """A bool per row -> ceil(n / 32) words, bit i % 32 of word i / 32 (the deleted-row layout)."""
    flags = np.asarray(flags, bool)
    padded = np.zeros(-(-flags.size // 32) * 32, bool)
    padded[:flags.size] = flags
    return np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").ravel()


def section_bytes(kind, count, dim, dtype) -> int:
    return {ROWS: count * dim * (2 if dtype == 1 else 4), NORMS: count * 4, DELETED: -(-count // 32) * 4, FILTER: -(-count // 32) * 4,
            LABELS: count * 4, TAGS: count * 8, VALUES: count * 8}[kind]


def encode_header(fields, table) -> bytes:
    """fields: version, dim, dtype, metric, count, live_count, id_offset, file_bytes, max_xn2_bits; table: (kind, offset,
    bytes, checksum) per section."""
    h = bytearray(BLOCK)
    h[:8] = MAGIC
    h[8:24] = np.array([fields["version"], fields["dim"], fields["dtype"], fields["metric"]], "<u4").tobytes()
    h[24:56] = np.array([fields["count"], fields["live_count"], fields["id_offset"], fields["file_bytes"]], "<u8").tobytes()
    h[56:64] = np.array([fields["max_xn2_bits"], len(table)], "<u4").tobytes()
    for i, (kind, off, nbytes, csum) in enumerate(table):
        at = TABLE_AT + i * ENTRY
        h[at:at + 8] = np.array([kind, 0], "<u4").tobytes()
        h[at + 8:at + 32] = np.array([off, nbytes, csum], "<u8").tobytes()
    h[SUM_AT:] = np.array([checksum(bytes(h[:SUM_AT]))], "<u8").tobytes()
    return bytes(h)


def write(path, *, dim, dtype, metric, rows, norms, deleted, id_offset=0, max_xn2_bits=0, allow=None, labels=None, tags=None,
          values=None, version=VERSION):
    """Write a snapshot.  rows: [count, dim] stored elements (uint16 bf16 bits or float32); norms: [count] f32; deleted /
    allow: a bool per row; labels u32, tags u64, values i64 per row, or None = the section is absent.
    -> {kind: (offset, bytes)} of the sections written."""
    count = int(np.asarray(rows).shape[0])
    deleted = np.asarray(deleted, bool)
    payloads = [(ROWS, np.ascontiguousarray(rows, "<u2" if dtype == 1 else "<f4").tobytes()),
                (NORMS, np.ascontiguousarray(norms, "<f4").tobytes()),
                (DELETED, pack_bits(deleted).tobytes())]
    if allow is not None:
        payloads.append((FILTER, pack_bits(allow).tobytes()))
    if labels is not None:
        payloads.append((LABELS, np.ascontiguousarray(labels, "<u4").tobytes()))
    if tags is not None:
        payloads.append((TAGS, np.ascontiguousarray(tags, "<u8").tobytes()))
    if values is not None:
        payloads.append((VALUES, np.ascontiguousarray(values, "<i8").tobytes()))
    table, body, at = [], bytearray(), BLOCK
    for kind, p in payloads:
        assert len(p) == section_bytes(kind, count, dim, dtype), kind
        table.append((kind, at, len(p), checksum(p)))
        body += p + b"\0" * (-len(p) % BLOCK)
        at += len(p) + (-len(p) % BLOCK)
    fields = dict(version=version, dim=dim, dtype=dtype, metric=metric, count=count, live_count=count - int(deleted.sum()),
                  id_offset=id_offset, file_bytes=at, max_xn2_bits=max_xn2_bits)
    with open(path, "wb") as f:
        f.write(encode_header(fields, table) + bytes(body))
    return {kind: (off, nbytes) for kind, off, nbytes, _ in table}


def read(path) -> dict:
    """Parse a snapshot and check everything the format promises: the magic, both kinds of checksum, offsets on 4096-byte
    boundaries in ascending order, section sizes that follow from count / dim / dtype, zero padding, the file's length.
    -> the header's fields, "sections": {kind: payload bytes}, "table": {kind: (offset, bytes, checksum)}."""
    raw = open(path, "rb").read()
    h = raw[:BLOCK]
    assert len(h) == BLOCK and h[:8] == MAGIC
    version, dim, dtype, metric = (int(v) for v in np.frombuffer(h, "<u4", 4, 8))
    count, live_count, id_offset, file_bytes = (int(v) for v in np.frombuffer(h, "<u8", 4, 24))
    max_xn2_bits, n_sections = (int(v) for v in np.frombuffer(h, "<u4", 2, 56))
    assert version == VERSION and file_bytes == len(raw)
    assert int(np.frombuffer(h, "<u8", 1, SUM_AT)[0]) == checksum(h[:SUM_AT]), "header checksum"
    assert not any(h[TABLE_AT + n_sections * ENTRY:SUM_AT]), "the rest of the header is not zero"
    sections, table, at = {}, {}, BLOCK
    for i in range(n_sections):
        e = TABLE_AT + i * ENTRY
        kind, zero = (int(v) for v in np.frombuffer(h, "<u4", 2, e))
        off, nbytes, csum = (int(v) for v in np.frombuffer(h, "<u8", 3, e + 8))
        assert zero == 0 and kind not in sections and off == at and off % BLOCK == 0, (kind, off, at)
        assert nbytes == section_bytes(kind, count, dim, dtype), (kind, nbytes)
        payload = raw[off:off + nbytes]
        assert checksum(payload) == csum, f"checksum of section {kind}"
        at = off + nbytes + (-nbytes % BLOCK)
        assert not any(raw[off + nbytes:at]), f"padding of section {kind} is not zero"
        sections[kind], table[kind] = payload, (off, nbytes, csum)
    assert at == len(raw)
    assert {ROWS, NORMS, DELETED} <= set(sections)
    return dict(version=version, dim=dim, dtype=dtype, metric=metric, count=count, live_count=live_count, id_offset=id_offset,
                file_bytes=file_bytes, max_xn2_bits=max_xn2_bits, sections=sections, table=table, raw=raw)
