"""A plain-Python model of the row keys (include/vrod.h "Row keys"), layered on index_model.ModelIndex: a list of keys
beside the rows, a dict for find, upsert as update-or-add.  Plus what the key tests share: the hash of keys_plan.h
restated in numpy, a search for keys with chosen low hash bits, a host rendering of the table's load rule, and helpers
that read and forge the key section of a snapshot by offsets (snapshot_model's checksum and encode_header).

numpy and the CPU oracle only; no GPU and no import of the library.
"""
import numpy as np

import snapshot_model as M
from index_model import ERR_INVALID_ARG, ERR_INVALID_VALUE, ModelError, ModelIndex
from support import ID_NONE

NONE = int(ID_NONE)
MASK = (1 << 64) - 1
MIN_SLOTS = 1024                                   # kKeyMinSlots
SNAP_KEYS = 8                                      # the snapshot section kind of the key column: [count] u64


# ---------------------------------------------------------------- the hash and the sizing rule, restated
def key_hash(keys) -> np.ndarray:
    """keys_plan.h key_hash over a uint64 array-like (all arithmetic mod 2^64)."""
    z = np.asarray(keys, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def key_hash_int(key: int) -> int:
    """The same in Python integers: an independent second statement of the contract."""
    z = (key + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def home(keys, slots) -> np.ndarray:
    return key_hash(keys) & np.uint64(slots - 1)


def table_slots(n, cur=0) -> int:
    """keys_plan.h key_table_slots: doubled from max(cur, 1024) until n keys fit in a quarter."""
    s = max(cur, MIN_SLOTS)
    while n > s // 4:
        s *= 2
    return s


def keys_with_low_bits(n, bits, value, start=1) -> np.ndarray:
    """The first n keys >= start whose hash has `value` in its low `bits` bits: they share a home in every table of up
    to 2**bits slots."""
    out = []
    at = start
    want, mask = np.uint64(value), np.uint64((1 << bits) - 1)
    while len(out) < n:
        cand = np.arange(at, at + (1 << 20), dtype=np.uint64)
        out.extend(int(k) for k in cand[(key_hash(cand) & mask) == want][:n - len(out)])
        at += 1 << 20
    return np.array(out, dtype=np.uint64)


# ---------------------------------------------------------------- the model
class KeysModel(ModelIndex):
    """ModelIndex plus one key per row (NONE until set), unique among the live rows."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.keys = np.zeros(0, np.uint64)
        self.keys_set = False                        # whether set_keys (or upsert) ever succeeded with n > 0

    def add(self, raw):
        grew = super().add(raw)
        self.keys = np.concatenate([self.keys, np.full(self.count - self.keys.size, ID_NONE, np.uint64)])
        return grew

    def compact(self, map_len=None):
        keep = ~self.deleted
        new_ids = super().compact(map_len)
        self.keys = self.keys[keep]
        return new_ids

    def holders(self) -> dict:
        """key -> local row, over the live keyed rows."""
        return {int(k): r for r, k in enumerate(self.keys) if not self.deleted[r] and int(k) != NONE}

    def keyed_live(self) -> int:
        return len(self.holders())

    def set_keys(self, first_id, keys):
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
        first = int(first_id) - self.offset
        if first < 0 or first > self.count or keys.size > self.count - first:
            raise ModelError(ERR_INVALID_ARG, "set_keys: a range past the rows")
        if keys.size == 0:
            return
        live = [int(k) for i, k in enumerate(keys) if not self.deleted[first + i] and int(k) != NONE]
        if len(set(live)) != len(live):
            raise ModelError(ERR_INVALID_ARG, "set_keys: a key given to two live rows")
        held = self.holders()
        for k in live:
            if k in held and not first <= held[k] < first + keys.size:
                raise ModelError(ERR_INVALID_ARG, "set_keys: a key held by a live row outside the range")
        self.keys = self.keys.copy()
        self.keys[first:first + keys.size] = keys
        self.keys_set = True

    def get_keys(self, first_id, n):
        first = int(first_id) - self.offset
        return self.keys[first:first + n].copy()

    def find_keys(self, keys) -> np.ndarray:
        held = self.holders()
        return np.array([held[int(k)] + self.offset if int(k) in held else NONE for k in np.asarray(keys, np.uint64).reshape(-1)],
                        dtype=np.uint64)

    def ids_to_keys(self, ids) -> np.ndarray:
        ids = np.asarray(ids, dtype=np.uint64)
        out = np.full(ids.shape, ID_NONE, np.uint64)
        flat, o = ids.reshape(-1), out.reshape(-1)
        for i, v in enumerate(flat):
            r = int(v) - self.offset
            if int(v) != NONE and 0 <= r < self.count:
                o[i] = self.keys[r]
        return out

    def delete(self, ids):
        super().delete(ids)

    def delete_keys(self, keys) -> int:
        found = self.find_keys(keys)
        rows = np.unique(found[found != ID_NONE])
        if rows.size:
            self.delete(rows)
        return int(rows.size)

    def upsert(self, keys, raw) -> np.ndarray:
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
        raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, self.dim)
        if keys.size == 0:
            return np.zeros(0, np.uint64)
        if (keys == ID_NONE).any() or np.unique(keys).size != keys.size:
            raise ModelError(ERR_INVALID_ARG, "upsert: no key, or a key twice")
        if not np.isfinite(raw).all():
            raise ModelError(ERR_INVALID_VALUE, "upsert: NaN or Inf")
        ids = self.find_keys(keys)
        old = ids != ID_NONE
        new = np.flatnonzero(~old)
        ids[new] = np.arange(self.count, self.count + new.size, dtype=np.uint64) + np.uint64(self.offset)
        if old.any():
            self.update(ids[old], raw[old])
        if new.size:
            first = self.count + self.offset
            self.add(raw[new])
            self.set_keys(first, keys[new])
        return ids


class TableModel:
    """A host rendering of the table's bookkeeping (not of its layout): which keys have a slot, and when the load rule
    rebuilds.  occupied counts stale slots, as vrod_key_stats does."""

    def __init__(self):
        self.slots, self.rebuilds, self.slotted = 0, 0, set()

    @property
    def occupied(self):
        return len(self.slotted)

    def insert(self, live_keys_before: int, incoming, live_keys_after):
        """A successful set of `incoming` keys (those of live rows, no NONE); live_keys_after: every live key afterwards."""
        incoming = [int(k) for k in incoming]
        first = self.slots == 0
        if first or self.occupied + len(incoming) > self.slots // 2:
            self.slots = table_slots(live_keys_before + len(incoming), self.slots)
            self.slotted = {int(k) for k in live_keys_after}
            self.rebuilds += 0 if first else 1
        else:
            self.slotted |= set(incoming)

    def rebuild(self, live_keys):
        self.slots = table_slots(len(live_keys), self.slots)
        self.slotted = {int(k) for k in live_keys}
        self.rebuilds += 1


# ---------------------------------------------------------------- a snapshot's key section, by offsets
def snapshot_table(raw):
    """The header of a snapshot's bytes -> (its fields as snapshot_model.encode_header takes them, its section table as a
    list of (kind, offset, bytes, checksum)).  snapshot_model.read knows the section kinds of its day only."""
    assert raw[:8] == M.MAGIC and int(np.frombuffer(raw, "<u8", 1, M.SUM_AT)[0]) == M.checksum(raw[:M.SUM_AT]), "header"
    version, dim, dtype, metric = (int(v) for v in np.frombuffer(raw, "<u4", 4, 8))
    count, live_count, id_offset, file_bytes = (int(v) for v in np.frombuffer(raw, "<u8", 4, 24))
    max_xn2_bits, n_sections = (int(v) for v in np.frombuffer(raw, "<u4", 2, 56))
    assert file_bytes == len(raw)
    table = []
    for i in range(n_sections):
        e = M.TABLE_AT + i * M.ENTRY
        off, nbytes, csum = (int(v) for v in np.frombuffer(raw, "<u8", 3, e + 8))
        table.append((int(np.frombuffer(raw, "<u4", 1, e)[0]), off, nbytes, csum))
    fields = dict(version=version, dim=dim, dtype=dtype, metric=metric, count=count, live_count=live_count, id_offset=id_offset,
                  file_bytes=file_bytes, max_xn2_bits=max_xn2_bits)
    return fields, table


def snapshot_keys(path):
    """The key column of a snapshot as uint64 (its checksum and size checked), or None if the file has no key section."""
    raw = open(path, "rb").read()
    fields, table = snapshot_table(raw)
    for kind, off, nbytes, csum in table:
        if kind == SNAP_KEYS:
            payload = raw[off:off + nbytes]
            assert nbytes == fields["count"] * 8 and off % M.BLOCK == 0 and M.checksum(payload) == csum
            return np.frombuffer(payload, "<u8").copy()
    return None


def forge_keys(src, dst, new_keys):
    """Copy snapshot `src` to `dst` with its key section replaced by new_keys ([count] uint64) and both checksums -- the
    section's and the header's -- made right: a file that is sound in every respect the format checks."""
    raw = bytearray(open(src, "rb").read())
    fields, table = snapshot_table(bytes(raw))
    payload = np.ascontiguousarray(new_keys, dtype="<u8").tobytes()
    at = [i for i, t in enumerate(table) if t[0] == SNAP_KEYS]
    assert at, "the snapshot has no key section"
    kind, off, nbytes, _ = table[at[0]]
    assert nbytes == len(payload)
    raw[off:off + nbytes] = payload
    table[at[0]] = (kind, off, nbytes, M.checksum(payload))
    raw[:M.BLOCK] = M.encode_header(fields, table)
    with open(dst, "wb") as f:
        f.write(raw)
