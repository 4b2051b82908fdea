"""Python harness over the C ABI (include/vrod.h): device memory plumbing only.

`Index` owns one `vrod_index*` (one GPU).  numpy in / numpy out goes through
`vrod_search`; torch device tensors go through `vrod_search_device` (torch is plumbing
here: device buffers, streams and torch.distributed for the RCCL all-gather).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import DupStats, KeyStats, MultivecStats, NearStats, RowfindStats, SearchStats, SnapshotInfo, VrodError, check

DTYPE_F32, DTYPE_BF16 = 0, 1
SRC_F32, SRC_BF16, SRC_F16 = 0, 1, 2   # vrod_src_dtype: the element type of rows given in device memory
METRIC_COSINE, METRIC_L2, METRIC_IP = 0, 1, 2
PATH_AUTO, PATH_STREAM, PATH_MFMA, PATH_EXACT, PATH_GATHER = 0, 1, 2, 3, 4
ID_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_K = 3584
BYID_EXCLUDE_SELF = 1   # VROD_BYID_EXCLUDE_SELF
MAX_QUERY_VECTORS = 256   # VROD_MAX_QUERY_VECTORS
MAX_DIVERSE_POOL = 1024   # VROD_MAX_DIVERSE_POOL
MAX_COMBINE_TERMS = 256   # VROD_MAX_COMBINE_TERMS
MAX_EXCLUDE = 1024        # VROD_MAX_EXCLUDE
COMBINED_EXCLUDE_TERMS = 1   # VROD_COMBINED_EXCLUDE_TERMS
MAX_CANDIDATES = 16384    # VROD_MAX_CANDIDATES
# vrod_where: one query's predicate of search_where, 40 bytes
WHERE_DTYPE = np.dtype([("any", np.uint64), ("all", np.uint64), ("none", np.uint64), ("lo", np.int64), ("hi", np.int64)])
# vrod_row_pred: the predicate of the row-predicate operations (count_where ... set_tags_where), 48 bytes
ROWPRED_DTYPE = np.dtype([("any", np.uint64), ("all", np.uint64), ("none", np.uint64), ("lo", np.int64), ("hi", np.int64),
                          ("label", np.uint32), ("has_label", np.uint32)])
ROWPRED_ALLOWED = 1   # VROD_ROWPRED_ALLOWED: only the rows the filter allows are in scope
ORDER_DESC = 2        # VROD_ORDER_DESC: value descending (ids still ascending among equal values)
MAX_ORDERED = 65536   # VROD_MAX_ORDERED: rows one select_ordered call returns
# vrod_order_cursor: the (value, id) a page ended with, 16 bytes
ORDER_CURSOR_DTYPE = np.dtype([("value", np.int64), ("id", np.uint64)])
AGG_BY_LABEL, AGG_BY_VALUE, AGG_BY_TAG = 0, 1, 2   # VROD_AGG_BY_*: the key of aggregate_where's groups
AGG_ORDER_COUNT = 4        # VROD_AGG_ORDER_COUNT: groups by count descending, then key (the flags word of ROWPRED_ALLOWED)
MAX_AGG_GROUPS = 1048576   # VROD_MAX_AGG_GROUPS: distinct groups one aggregate_where call holds
# vrod_agg_group: one group of aggregate_where, 48 bytes
AGG_GROUP_DTYPE = np.dtype([("key", np.int64), ("count", np.uint64), ("min_value", np.int64), ("max_value", np.int64),
                            ("sum_value", np.int64), ("first_id", np.uint64)])
CENTROID_SUM = 8               # VROD_CENTROID_SUM: centroids_where writes each group's sum, not its mean (the flags word of ROWPRED_ALLOWED)
MAX_CENTROID_GROUPS = 65536    # VROD_MAX_CENTROID_GROUPS: groups one centroids_where call holds
# vrod_centroid_group: one group of centroids_where, 24 bytes
CENTROID_GROUP_DTYPE = np.dtype([("key", np.int64), ("count", np.uint64), ("first_id", np.uint64)])
DUP_WITHIN_LABEL = 1            # VROD_DUP_WITHIN_LABEL: the class key is (label, row bits)
DUP_NARROW_HASH = 0x80000000    # VROD_DUP_NARROW_HASH: a diagnostic, the row hash cut to 8 bits
ROWFIND_NARROW_HASH = 0x80000000   # VROD_ROWFIND_NARROW_HASH: a diagnostic, the row hash cut to 8 bits
ROWFIND_SMALL_BATCH = 0x40000000   # VROD_ROWFIND_SMALL_BATCH: a diagnostic, lookup batches of 96 rows
NEAR_SMALL_POOL = 0x80000000   # VROD_NEAR_SMALL_POOL: a diagnostic, the hit pool cut to the eligible-row count
# rows per batch of knn_graph() by storage type (byid_plan.h: kByidBatchF32, kByidBatchBf16)
KNN_BATCH = {0: 256, 1: 1024}

_DTYPES = {"f32": DTYPE_F32, "fp32": DTYPE_F32, "float32": DTYPE_F32, "bf16": DTYPE_BF16, "bfloat16": DTYPE_BF16}
_METRICS = {"cosine": METRIC_COSINE, "cos": METRIC_COSINE, "l2": METRIC_L2, "euclidean": METRIC_L2,
            "ip": METRIC_IP, "dot": METRIC_IP, "inner_product": METRIC_IP}


def _enum(v, table, what):
    if isinstance(v, str):
        try:
            return table[v.lower()]
        except KeyError:
            raise ValueError(f"unknown {what} {v!r}") from None
    return int(v)


def _ptr(a):
    """The data pointer of a numpy array; None (a NULL pointer) stays None."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _out(nq, k, *dtypes):
    """One empty [nq, k] numpy result array per dtype."""
    return tuple(np.empty((nq, k), dtype=d) for d in dtypes)


def _device_out(out, shape, dtype, device):
    """The caller's output tensor, or a new one of `shape`."""
    if out is None:
        import torch
        out = torch.empty(shape, dtype=dtype, device=device)
    return out


class Index:
    """One shard of a brute-force index on one MI355X."""

    def __init__(self, dim: int, dtype="f32", metric="cosine", device: int = 0, devices=None):
        """`devices` (a list of device ids, repeats allowed) makes ONE handle that deals its rows to
        several GPUs and searches them all per call (vrod_index_create with n_devices > 1)."""
        self._L = _lib.load()
        self._h = C.c_void_p()
        self.dim = int(dim)
        self.dtype = _enum(dtype, _DTYPES, "dtype")
        self.metric = _enum(metric, _METRICS, "metric")
        ids = [int(d) for d in devices] if devices is not None else [int(device)]
        self.device = ids[0]
        dev = (C.c_int * len(ids))(*ids)
        check(self._L.vrod_index_create(C.byref(self._h), self.dim, self.dtype, self.metric, dev, len(ids)))

    # -- snapshots
    def save(self, path):
        """Write the handle's whole observable state to `path` (vrod_index_save): atomic, deterministic bytes."""
        check(self._L.vrod_index_save(self._h, os.fsencode(path)))

    @classmethod
    def load(cls, path, device: int = 0):
        """A new handle from a snapshot (vrod_index_load): it answers every call as the saved one did, to the bit."""
        self = cls.__new__(cls)
        self._L = _lib.load()
        self._h = C.c_void_p()
        self.device = int(device)
        dev = (C.c_int * 1)(self.device)
        check(self._L.vrod_index_load(C.byref(self._h), os.fsencode(path), dev, 1))
        info = snapshot_info(path)
        self.dim, self.dtype, self.metric = info["dim"], info["dtype"], info["metric"]
        self._id_offset = info["id_offset"]
        return self

    # -- lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.vrod_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- corpus
    def reserve(self, n: int):
        check(self._L.vrod_index_reserve(self._h, int(n)))

    def add(self, rows: np.ndarray):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        check(self._L.vrod_index_add(self._h, _ptr(rows), rows.shape[0]))

    def add_synthetic(self, seed: int, first_row: int, n: int):
        check(self._L.vrod_index_add_synthetic(self._h, int(seed), int(first_row), int(n)))

    @property
    def count(self) -> int:
        out = C.c_uint64()
        check(self._L.vrod_index_count(self._h, C.byref(out)))
        return out.value

    @staticmethod
    def _ids(ids) -> np.ndarray:
        """Any integer array-like -> a contiguous uint64 vector."""
        a = np.asarray(ids)
        if a.size and a.dtype.kind not in "iu" and not isinstance(ids, np.ndarray):
            # a sequence of Python ints that numpy could not give one integer dtype (e.g. 1 and 2**63 together)
            flat = list(np.asarray(ids, dtype=object).reshape(-1))
            if all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in flat):
                a = np.array([int(x) for x in flat], dtype=np.uint64)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"ids must be integers, got {a.dtype}")
        return np.ascontiguousarray(a.astype(np.uint64, copy=False).reshape(-1))

    def delete(self, ids):
        """Delete rows by the ids searches report (vrod_index_delete): any integer array-like, all or nothing."""
        a = self._ids(ids)
        check(self._L.vrod_index_delete(self._h, _ptr(a), a.size))

    def update(self, ids, rows: np.ndarray):
        """Give row ids[i] the vector rows[i] in place (vrod_index_update): the row keeps its id, the vector is prepared
        as add() prepares it.  All or nothing; an id named twice takes the last vector."""
        a = self._ids(ids)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim == 1 and a.size == 1:
            rows = rows[None, :]
        if rows.ndim != 2 or rows.shape[1] != self.dim or rows.shape[0] != a.size:
            raise ValueError(f"rows must be [{a.size}, {self.dim}]")
        check(self._L.vrod_index_update(self._h, _ptr(a), _ptr(rows), a.size))

    def compact(self) -> np.ndarray:
        """Physically remove the deleted rows and renumber the survivors densely (vrod_index_compact).  Returns the
        new-id map, a uint64 array over the old rows: entry i is the new id of old id offset + i, or ID_NONE."""
        n = self.count
        new_ids = np.empty(n, dtype=np.uint64)
        check(self._L.vrod_index_compact(self._h, _ptr(new_ids), n))
        return new_ids

    def live_count(self) -> int:
        """Rows added minus rows deleted."""
        out = C.c_uint64()
        check(self._L.vrod_index_live_count(self._h, C.byref(out)))
        return out.value

    def set_filter(self, allow):
        """Allow-list filter (vrod_index_set_filter): a bool array-like of length <= count() -- entry i True = id
        offset + i may be returned -- or None to clear.  Every later search returns only rows that are live and allowed;
        rows past the array (rows added later included) are not allowed."""
        if allow is None:
            check(self._L.vrod_index_set_filter(self._h, None, 0))
            return
        a = np.asarray(allow)
        if a.dtype != np.bool_:
            raise TypeError(f"allow must be a bool array, got {a.dtype}")
        a = a.reshape(-1)
        n = a.size
        buf = np.zeros(max(1, (n + 31) // 32) * 4, np.uint8)   # bit i % 32 of word i / 32 (a little-endian host)
        packed = np.packbits(a, bitorder="little")
        buf[:packed.size] = packed
        words = buf.view(np.uint32)
        check(self._L.vrod_index_set_filter(self._h, _ptr(words), n))

    def filter_count(self) -> int:
        """Rows the next search may return: live and allowed (= live_count() without a filter)."""
        out = C.c_uint64()
        check(self._L.vrod_index_filter_count(self._h, C.byref(out)))
        return out.value

    @staticmethod
    def _labels(labels, n=None) -> np.ndarray:
        """An integer array-like of labels (each in 0 .. 2**32 - 1; `n` of them when given) -> a contiguous uint32 vector."""
        a = np.asarray(labels)
        if a.dtype.kind not in "iu" and (a.size or isinstance(labels, np.ndarray)):   # (an empty list has no dtype of its own)
            raise TypeError(f"labels must be an integer array, got {a.dtype}")
        a = a.reshape(-1)
        if n is not None and a.size != n:
            raise ValueError(f"labels must hold {n} values, got {a.size}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("labels must fit 32 unsigned bits")
        return np.ascontiguousarray(a.astype(np.uint32, copy=False))

    def set_labels(self, first_id: int, labels):
        """Give the rows with ids first_id, first_id + 1, ... the labels of an integer array-like (vrod_index_set_labels).
        Every row carries label 0 until it is given one; only search_labeled and search_grouped read labels."""
        a = self._labels(labels)
        check(self._L.vrod_index_set_labels(self._h, int(first_id), _ptr(a), a.size))

    def get_labels(self, first_id: int, n: int) -> np.ndarray:
        out = np.empty(int(n), dtype=np.uint32)
        check(self._L.vrod_index_get_labels(self._h, int(first_id), int(n), _ptr(out)))
        return out

    @staticmethod
    def _u64(values, what, shape) -> np.ndarray:
        """An integer array-like of 64-bit masks -> a contiguous uint64 array of `shape` (-1: any length)."""
        a = np.asarray(values)
        if a.dtype.kind not in "iu" and (a.size or isinstance(values, np.ndarray)):   # (an empty list has no dtype of its own)
            raise TypeError(f"{what} must be an integer array, got {a.dtype}")
        if a.dtype != np.uint64:
            if a.size and int(a.min()) < 0:
                raise ValueError(f"{what} must fit 64 unsigned bits")
            a = a.astype(np.uint64)
        try:
            a = a.reshape(shape)
        except ValueError:
            raise ValueError(f"{what} must have shape {shape}, got {a.shape}") from None
        return np.ascontiguousarray(a)

    def set_tags(self, first_id: int, tags):
        """Give the rows with ids first_id, first_id + 1, ... the 64-bit tag masks of an integer array-like
        (vrod_index_set_tags).  Every row carries 0 until it is given tags; only search_tagged reads them."""
        a = self._u64(tags, "tags", (-1,))
        check(self._L.vrod_index_set_tags(self._h, int(first_id), _ptr(a), a.size))

    def get_tags(self, first_id: int, n: int) -> np.ndarray:
        out = np.empty(int(n), dtype=np.uint64)
        check(self._L.vrod_index_get_tags(self._h, int(first_id), int(n), _ptr(out)))
        return out

    @staticmethod
    def _i64(values, what) -> np.ndarray:
        """An integer array-like of signed 64-bit values -> a contiguous int64 vector."""
        a = np.asarray(values)
        if a.dtype.kind not in "iu" and (a.size or isinstance(values, np.ndarray)):   # (an empty list has no dtype of its own)
            raise TypeError(f"{what} must be an integer array, got {a.dtype}")
        if a.dtype.kind == "u" and a.size and int(a.max()) > 0x7FFFFFFFFFFFFFFF:
            raise ValueError(f"{what} must fit 64 signed bits")
        return np.ascontiguousarray(a.reshape(-1).astype(np.int64, copy=False))

    def set_values(self, first_id: int, values):
        """Give the rows with ids first_id, first_id + 1, ... the signed 64-bit values of an integer array-like
        (vrod_index_set_values).  Every row carries 0 until it is given a value; only search_where reads them."""
        a = self._i64(values, "values")
        check(self._L.vrod_index_set_values(self._h, int(first_id), _ptr(a), a.size))

    def get_values(self, first_id: int, n: int) -> np.ndarray:
        out = np.empty(int(n), dtype=np.int64)
        check(self._L.vrod_index_get_values(self._h, int(first_id), int(n), _ptr(out)))
        return out

    # -- row keys
    @classmethod
    def _keys(cls, keys) -> np.ndarray:
        """An integer array-like of keys (each in 0 .. 2**64 - 1, ID_NONE included) -> a contiguous uint64 vector."""
        a = np.asarray(keys)
        if a.dtype.kind == "i" and a.size and int(a.min()) < 0:
            raise ValueError("keys must fit 64 unsigned bits")
        return cls._ids(keys)

    def set_keys(self, first_id: int, keys):
        """Give the rows with ids first_id, first_id + 1, ... the caller's 64-bit keys (vrod_index_set_keys).  Every row
        carries ID_NONE ("no key") until it is given one; no two live rows may hold the same key.  No search reads keys."""
        a = self._keys(keys)
        check(self._L.vrod_index_set_keys(self._h, int(first_id), _ptr(a), a.size))

    def get_keys(self, first_id: int, n: int) -> np.ndarray:
        out = np.empty(int(n), dtype=np.uint64)
        check(self._L.vrod_index_get_keys(self._h, int(first_id), int(n), _ptr(out)))
        return out

    def find_keys(self, keys) -> np.ndarray:
        """keys -> the ids of the live rows that hold them, ID_NONE where no live row does (vrod_index_find_keys)."""
        a = self._keys(keys)
        out = np.empty(a.size, dtype=np.uint64)
        check(self._L.vrod_index_find_keys(self._h, _ptr(a), a.size, _ptr(out)))
        return out

    def ids_to_keys(self, ids) -> np.ndarray:
        """ids (any shape, e.g. a search's [nq, k]) -> the keys their rows store, ID_NONE for ID_NONE, an id that is no
        current row, or a row without a key (vrod_index_ids_to_keys)."""
        flat = self._ids(ids)
        out = np.empty(flat.size, dtype=np.uint64)
        check(self._L.vrod_index_ids_to_keys(self._h, _ptr(flat), flat.size, _ptr(out)))
        return out.reshape(np.shape(ids))

    def _device_u64(self, t, what):
        """Checks a device tensor of 64-bit words (int64, the bits of uint64) -> (its element count, its device's stream)."""
        import torch
        if t.dtype != torch.int64:
            raise TypeError(f"{what} must be an int64 tensor, got {t.dtype}")
        assert t.is_cuda and t.is_contiguous()
        return t.numel(), C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def find_keys_device(self, d_keys, out_ids=None):
        """torch CUDA tensor of keys (int64, the bits of uint64, any shape) -> the ids (same shape), complete on return."""
        import torch
        n, stream = self._device_u64(d_keys, "keys")
        out_ids = _device_out(out_ids, tuple(d_keys.shape), torch.int64, d_keys.device)
        check(self._L.vrod_index_find_keys_device(self._h, d_keys.data_ptr(), n, out_ids.data_ptr(), stream))
        return out_ids

    def ids_to_keys_device(self, d_ids, out_keys=None):
        """torch CUDA tensor of ids (int64-viewed-uint64, e.g. search_device's [nq, k]) -> the keys (same shape), complete
        on return: a result list becomes the caller's names without leaving the device."""
        import torch
        n, stream = self._device_u64(d_ids, "ids")
        out_keys = _device_out(out_keys, tuple(d_ids.shape), torch.int64, d_ids.device)
        check(self._L.vrod_index_ids_to_keys_device(self._h, d_ids.data_ptr(), n, out_keys.data_ptr(), stream))
        return out_keys

    def delete_keys(self, keys) -> int:
        """Delete the live row of each key; keys no live row holds are ignored (vrod_index_delete_keys).  -> rows that died."""
        a = self._keys(keys)
        out = C.c_uint64()
        check(self._L.vrod_index_delete_keys(self._h, _ptr(a), a.size, C.byref(out)))
        return out.value

    def upsert(self, keys, rows: np.ndarray) -> np.ndarray:
        """Row of keys[i] := rows[i]: updated in place where a live row holds the key, appended and keyed otherwise
        (vrod_index_upsert).  All or nothing.  -> each key's id."""
        a = self._keys(keys)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim == 1 and a.size == 1:
            rows = rows[None, :]
        if rows.ndim != 2 or rows.shape[1] != self.dim or rows.shape[0] != a.size:
            raise ValueError(f"rows must be [{a.size}, {self.dim}]")
        out = np.empty(a.size, dtype=np.uint64)
        check(self._L.vrod_index_upsert(self._h, _ptr(a), _ptr(rows), a.size, _ptr(out)))
        return out

    # -- device-resident ingest
    def _device_rows(self, t, what="rows"):
        """Checks a source (or destination) of rows in GPU memory: a 2-D CUDA tensor [n, dim] of float32, bfloat16 or
        float16 whose rows are contiguous (stride(1) == 1) and stride(0) >= dim apart -- a row or column slice of a
        larger tensor is fine.  -> (n, the vrod_src_dtype, stride(0), its device's current stream)."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what} must be a torch tensor, got {type(t).__name__}")
        src = {torch.float32: SRC_F32, torch.bfloat16: SRC_BF16, torch.float16: SRC_F16}.get(t.dtype)
        if src is None:
            raise ValueError(f"{what} must be float32, bfloat16 or float16, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError(f"{what} must be [n, {self.dim}], got {tuple(t.shape)}")
        n = t.shape[0]
        stride = t.stride(0) if n > 1 else max(t.stride(0), self.dim)   # (a single row's stride is never used)
        if self.dim > 1 and t.stride(1) != 1:
            raise ValueError(f"{what} must have contiguous rows (stride(1) == 1), got stride {t.stride(1)}")
        if stride < self.dim:
            raise ValueError(f"{what} must have stride(0) >= {self.dim}, got {t.stride(0)}")
        if not t.is_cuda:
            raise ValueError(f"{what} must be a tensor on the GPU, got device {t.device}")
        return n, src, stride, C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def add_device(self, t):
        """add() from a CUDA tensor [n, dim] (float32 / bfloat16 / float16, any row stride >= dim): the rows never touch
        the host (vrod_index_add_device).  The handle ends up exactly as add() of the widened rows leaves it."""
        n, src, stride, stream = self._device_rows(t)
        check(self._L.vrod_index_add_device(self._h, t.data_ptr(), src, stride, n, stream))

    def update_device(self, d_ids, t):
        """update() from a CUDA int64 tensor of ids (the bits of uint64) and a CUDA tensor of rows (vrod_index_update_device)."""
        n, src, stride, stream = self._device_rows(t)
        n_ids, _ = self._device_u64(d_ids, "ids")
        if n_ids != n:
            raise ValueError(f"rows must be [{n_ids}, {self.dim}]")
        check(self._L.vrod_index_update_device(self._h, d_ids.data_ptr(), t.data_ptr(), src, stride, n, stream))

    def upsert_device(self, d_keys, t, out_ids=None):
        """upsert() from a CUDA int64 tensor of keys and a CUDA tensor of rows (vrod_index_upsert_device) -> each key's id,
        a CUDA int64 tensor."""
        import torch
        n, src, stride, stream = self._device_rows(t)
        n_keys, _ = self._device_u64(d_keys, "keys")
        if n_keys != n:
            raise ValueError(f"rows must be [{n_keys}, {self.dim}]")
        out_ids = _device_out(out_ids, (n,), torch.int64, t.device)
        if out_ids.numel() != n:
            raise ValueError(f"out_ids must hold {n} ids")
        self._device_u64(out_ids, "out_ids")
        check(self._L.vrod_index_upsert_device(self._h, d_keys.data_ptr(), t.data_ptr(), src, stride, n, out_ids.data_ptr(), stream))
        return out_ids

    def get_rows_device(self, first: int, n: int, out=None):
        """get_rows() into a CUDA float32 tensor [n, dim] (vrod_index_get_rows_device); `out` may be a strided view, the
        elements between its rows are not written."""
        import torch
        out = _device_out(out, (int(n), self.dim), torch.float32, torch.device("cuda", self.device))
        rows, src, stride, stream = self._device_rows(out, "out")
        if src != SRC_F32 or rows != int(n):
            raise ValueError(f"out must be a float32 tensor [{int(n)}, {self.dim}]")
        check(self._L.vrod_index_get_rows_device(self._h, int(first), int(n), out.data_ptr(), stride, stream))
        return out

    def key_stats(self) -> dict:
        """keyed_live, slots, occupied, rebuilds, max_probe of the key table (vrod_index_key_stats); zeros before set_keys."""
        st = KeyStats()
        check(self._L.vrod_index_key_stats(self._h, C.byref(st)))
        return st.as_dict()

    @classmethod
    def _where(cls, preds, nq) -> np.ndarray:
        """The predicates of search_where -> a contiguous [nq] array of WHERE_DTYPE (the layout of vrod_where).  preds is
        such a structured array, or an integer [nq, 5] array-like with the columns any, all, none (64 unsigned bits) and
        lo, hi (64 signed bits); Python ints keep both ranges, an int64 array's masks must not be negative, a uint64
        array's ends must fit 63 bits."""
        if isinstance(preds, np.ndarray) and preds.dtype.names:
            if preds.dtype != WHERE_DTYPE:
                raise TypeError(f"preds must have dtype {WHERE_DTYPE}, got {preds.dtype}")
            p = np.ascontiguousarray(preds.reshape(-1))
        else:
            a = preds if isinstance(preds, np.ndarray) else np.array(preds, dtype=object)   # (a list keeps its Python ints)
            if a.dtype == object and a.size:
                if not all(isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) for x in a.reshape(-1)):
                    raise TypeError("preds must hold integers")
            elif a.dtype.kind not in "iu" and (a.size or isinstance(preds, np.ndarray)):
                raise TypeError(f"preds must be an integer array, got {a.dtype}")
            if a.size == 0:
                a = np.zeros((0, 5), np.int64)
            if a.ndim != 2 or a.shape[1] != 5:
                raise ValueError(f"preds must have shape ({nq}, 5), got {a.shape}")
            p = np.empty(a.shape[0], WHERE_DTYPE)
            for j, name in enumerate(WHERE_DTYPE.names):
                col = a[:, j]
                if col.dtype == object:   # Python ints: the column's own range decides
                    try:
                        col = col.astype(np.uint64 if j < 3 else np.int64)
                    except OverflowError:
                        raise ValueError(f"preds column {name} does not fit 64 {'unsigned' if j < 3 else 'signed'} bits") from None
                p[name] = cls._u64(col, f"preds column {name}", (-1,)) if j < 3 else cls._i64(col, f"preds column {name}")
        if p.size != nq:
            raise ValueError(f"preds must hold {nq} predicates, got {p.size}")
        return p

    # -- row predicates
    @classmethod
    def _row_preds(cls, preds, n=None) -> np.ndarray:
        """The predicates of the row-predicate operations -> a contiguous array of ROWPRED_DTYPE (the layout of
        vrod_row_pred), `n` of them when given.  preds is such a structured array, or an integer [n, 7] array-like with the
        columns any, all, none (64 unsigned bits), lo, hi (64 signed bits), label (32 unsigned bits) and has_label (0 or
        1); one predicate may be given as its 7 values.  The ranges are checked as _where checks them."""
        if isinstance(preds, np.void):   # one element of a structured array
            preds = np.asarray(preds)
        if isinstance(preds, np.ndarray) and preds.dtype.names:
            if preds.dtype != ROWPRED_DTYPE:
                raise TypeError(f"preds must have dtype {ROWPRED_DTYPE}, got {preds.dtype}")
            p = np.ascontiguousarray(preds.reshape(-1))
        else:
            a = preds if isinstance(preds, np.ndarray) else np.array(preds, dtype=object)   # (a list keeps its Python ints)
            if a.dtype == object and a.size:
                if not all(isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) for x in a.reshape(-1)):
                    raise TypeError("preds must hold integers")
            elif a.dtype.kind not in "iu" and (a.size or isinstance(preds, np.ndarray)):
                raise TypeError(f"preds must be an integer array, got {a.dtype}")
            if a.size == 0:
                a = np.zeros((0, 7), np.int64)
            if a.ndim == 1 and a.shape[0] == 7:
                a = a.reshape(1, 7)
            if a.ndim != 2 or a.shape[1] != 7:
                raise ValueError(f"preds must have shape (n, 7), got {a.shape}")
            p = np.empty(a.shape[0], ROWPRED_DTYPE)
            for j, name in enumerate(ROWPRED_DTYPE.names):
                col = a[:, j]
                signed = j in (3, 4)
                if col.dtype == object:   # Python ints: the column's own range decides
                    try:
                        col = col.astype(np.int64 if signed else np.uint64)
                    except OverflowError:
                        raise ValueError(f"preds column {name} does not fit 64 {'signed' if signed else 'unsigned'} bits") from None
                if signed:
                    p[name] = cls._i64(col, f"preds column {name}")
                elif j < 3:
                    p[name] = cls._u64(col, f"preds column {name}", (-1,))
                else:
                    p[name] = cls._labels(col)
        if (p["has_label"] > 1).any():
            raise ValueError("has_label must be 0 or 1")
        if n is not None and p.size != n:
            raise ValueError(f"preds must hold {n} predicates, got {p.size}")
        return p

    @staticmethod
    def row_pred(any=0, all=0, none=0, lo=-(1 << 63), hi=(1 << 63) - 1, label=None) -> np.ndarray:   # noqa: A002
        """One predicate as a [1] array of ROWPRED_DTYPE; label=None: the label is not compared.  The defaults match every row."""
        return Index._row_preds([[any, all, none, lo, hi, 0 if label is None else label, 0 if label is None else 1]], 1)

    @staticmethod
    def _rowpred_flags(allowed_only) -> int:
        if not isinstance(allowed_only, (bool, np.bool_)):
            raise TypeError(f"allowed_only must be a bool, got {type(allowed_only).__name__}")
        return ROWPRED_ALLOWED if allowed_only else 0

    def count_where(self, preds, allowed_only: bool = False) -> np.ndarray:
        """preds (see _row_preds) -> uint64 [n]: the live rows (allowed_only: and allowed by the filter) matching each
        (vrod_index_count_where).  The columns are read on the device, 1024 distinct predicates per pass."""
        p = self._row_preds(preds)
        flags = self._rowpred_flags(allowed_only)
        out = np.zeros(p.size, dtype=np.uint64)
        check(self._L.vrod_index_count_where(self._h, _ptr(p), p.size, flags, _ptr(out)))
        return out

    def select_where(self, pred, allowed_only: bool = False, capacity=None) -> np.ndarray:
        """The ids of the rows in scope matching one predicate, ascending (vrod_index_select_where).  capacity=None: a
        count-only call sizes the buffer; else more than `capacity` matching rows raise VrodError with code ERR_CAPACITY
        (and .count holds the exact count)."""
        p = self._row_preds(pred, 1)
        flags = self._rowpred_flags(allowed_only)
        n = C.c_uint64()
        if capacity is None:
            rc = self._L.vrod_index_select_where(self._h, _ptr(p), flags, 0, C.byref(n), None)
            if rc not in (0, _lib.ERR_CAPACITY):
                check(rc)
            capacity = n.value
            if rc == 0:
                return np.empty(0, np.uint64)
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        ids = np.empty(max(capacity, 1), dtype=np.uint64)
        rc = self._L.vrod_index_select_where(self._h, _ptr(p), flags, capacity, C.byref(n), _ptr(ids) if capacity else None)
        if rc == _lib.ERR_CAPACITY:
            e = VrodError(rc, self._L.vrod_last_error().decode("utf-8", "replace"))
            e.count = n.value
            raise e
        check(rc)
        return ids[:n.value]

    def select_where_device(self, pred, capacity: int, allowed_only: bool = False, out_ids=None):
        """select_where into a CUDA int64 tensor [capacity] (the bits of uint64) -> (rc, count, ids): rc is 0 or
        ERR_CAPACITY, count is exact either way, ids[:count] are filled when rc is 0 (vrod_index_select_where_device).  The
        ids can feed search_candidates_device, update_device and ids_to_keys_device without a host trip."""
        import torch
        p = self._row_preds(pred, 1)
        flags = self._rowpred_flags(allowed_only)
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        dev = torch.device("cuda", self.device)
        out_ids = _device_out(out_ids, max(capacity, 1), torch.int64, dev)
        n_out, _ = self._device_u64(out_ids, "out_ids")
        if n_out < capacity:
            raise ValueError(f"out_ids must hold {capacity} ids")
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n = C.c_uint64()
        rc = self._L.vrod_index_select_where_device(self._h, _ptr(p), flags, capacity, C.byref(n), out_ids.data_ptr() if capacity else None, stream)
        if rc not in (0, _lib.ERR_CAPACITY):
            check(rc)
        return rc, n.value, out_ids

    def delete_where(self, pred, allowed_only: bool = False) -> int:
        """Delete every row in scope matching one predicate, as delete() of select_where's ids (vrod_index_delete_where).
        -> rows that died."""
        p = self._row_preds(pred, 1)
        flags = self._rowpred_flags(allowed_only)
        out = C.c_uint64()
        check(self._L.vrod_index_delete_where(self._h, _ptr(p), flags, C.byref(out)))
        return out.value

    def set_filter_where(self, pred, narrow: bool = False):
        """Make the rows matching one predicate the allow list, deleted rows included, as set_filter() of those bits
        (vrod_index_set_filter_where); narrow=True keeps only what the current filter allows as well.  The where-clause of
        every search form that honours the filter."""
        p = self._row_preds(pred, 1)
        flags = self._rowpred_flags(narrow)
        check(self._L.vrod_index_set_filter_where(self._h, _ptr(p), flags))

    def set_tags_where(self, pred, set_bits: int = 0, clear_bits: int = 0, allowed_only: bool = False) -> int:
        """tags := (tags & ~clear_bits) | set_bits on every row in scope matching one predicate (vrod_index_set_tags_where).
        -> rows whose mask changed."""
        p = self._row_preds(pred, 1)
        flags = self._rowpred_flags(allowed_only)
        for b in (set_bits, clear_bits):
            if not isinstance(b, (int, np.integer)) or isinstance(b, (bool, np.bool_)):
                raise TypeError("set_bits and clear_bits must be integers")
            if not 0 <= int(b) <= 0xFFFFFFFFFFFFFFFF:
                raise ValueError("set_bits and clear_bits must fit 64 unsigned bits")
        bits = (int(set_bits), int(clear_bits))
        if bits[0] & bits[1]:
            raise ValueError("set_bits and clear_bits share bits")
        out = C.c_uint64()
        check(self._L.vrod_index_set_tags_where(self._h, _ptr(p), flags, bits[0], bits[1], C.byref(out)))
        return out.value

    # -- ordered selection
    @classmethod
    def _order_args(cls, limit, desc, after, allowed_only):
        """The checked arguments of select_ordered -> (limit, flags, cursor): cursor is None or a [1] array of
        ORDER_CURSOR_DTYPE."""
        if not isinstance(desc, (bool, np.bool_)):
            raise TypeError(f"desc must be a bool, got {type(desc).__name__}")
        flags = cls._rowpred_flags(allowed_only) | (ORDER_DESC if desc else 0)
        if not isinstance(limit, (int, np.integer)) or isinstance(limit, (bool, np.bool_)):
            raise TypeError(f"limit must be an int, got {type(limit).__name__}")
        if not 0 <= int(limit) <= MAX_ORDERED:
            raise ValueError(f"limit must be in 0..{MAX_ORDERED}, got {limit}")
        cur = None
        if after is not None:
            if isinstance(after, np.void):   # one element of an ORDER_CURSOR_DTYPE array
                after = after.tolist()
            if not isinstance(after, (tuple, list)) or len(after) != 2:
                raise TypeError("after must be a (value, id) pair")
            for x in after:
                if not isinstance(x, (int, np.integer)) or isinstance(x, (bool, np.bool_)):
                    raise TypeError("after must hold two integers")
            v, i = int(after[0]), int(after[1])
            if not -(1 << 63) <= v < (1 << 63):
                raise ValueError("after: the value does not fit 64 signed bits")
            if not 0 <= i < (1 << 64):
                raise ValueError("after: the id does not fit 64 unsigned bits")
            cur = np.zeros(1, ORDER_CURSOR_DTYPE)
            cur["value"], cur["id"] = v, i
        return int(limit), flags, cur

    def select_ordered(self, pred, limit: int, desc: bool = False, after=None, allowed_only: bool = False):
        """The first `limit` rows in scope matching one predicate by (value, id) ascending -- desc: value descending, ids
        still ascending among equal values -- strictly after the cursor `after`, a (value, id) pair that need not name a
        row (vrod_index_select_ordered) -> (ids uint64 [n], values int64 [n], total): n = min(limit, total), total = the
        rows after the cursor.  limit=0 only counts."""
        p = self._row_preds(pred, 1)
        limit, flags, cur = self._order_args(limit, desc, after, allowed_only)
        ids, vals = np.empty(max(limit, 1), np.uint64), np.empty(max(limit, 1), np.int64)
        n, total = C.c_uint64(), C.c_uint64()
        check(self._L.vrod_index_select_ordered(self._h, _ptr(p), flags, _ptr(cur), limit, C.byref(n), C.byref(total),
                                                _ptr(ids) if limit else None, _ptr(vals) if limit else None))
        return ids[:n.value], vals[:n.value], total.value

    def select_ordered_device(self, pred, limit: int, desc: bool = False, after=None, allowed_only: bool = False, out_ids=None,
                              out_values=None):
        """select_ordered into CUDA int64 tensors [limit] (the ids are the bits of uint64) -> (count, total, ids, values);
        ids[:count] and values[:count] are filled (vrod_index_select_ordered_device).  The ids can feed
        search_candidates_device, update_device and ids_to_keys_device without a host trip."""
        import torch
        p = self._row_preds(pred, 1)
        limit, flags, cur = self._order_args(limit, desc, after, allowed_only)
        dev = torch.device("cuda", self.device)
        out_ids = _device_out(out_ids, max(limit, 1), torch.int64, dev)
        out_values = _device_out(out_values, max(limit, 1), torch.int64, dev)
        for t, name in ((out_ids, "out_ids"), (out_values, "out_values")):
            if self._device_u64(t, name)[0] < limit:
                raise ValueError(f"{name} must hold {limit} entries")
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n, total = C.c_uint64(), C.c_uint64()
        check(self._L.vrod_index_select_ordered_device(self._h, _ptr(p), flags, _ptr(cur), limit, C.byref(n), C.byref(total),
                                                       out_ids.data_ptr() if limit else None, out_values.data_ptr() if limit else None, stream))
        return n.value, total.value, out_ids, out_values

    def scroll(self, pred, page: int, desc: bool = False, allowed_only: bool = False):
        """A generator of select_ordered pages of up to `page` rows, (ids, values) each, the last (value, id) of one page
        being the cursor of the next: the whole listing in order.  Rows may be added, deleted and compacted between pages;
        every page is exact for the handle's state when it is fetched."""
        if not isinstance(page, (int, np.integer)) or isinstance(page, (bool, np.bool_)):
            raise TypeError(f"page must be an int, got {type(page).__name__}")
        if not 1 <= int(page) <= MAX_ORDERED:
            raise ValueError(f"page must be in 1..{MAX_ORDERED}, got {page}")
        self._row_preds(pred, 1)
        self._order_args(int(page), desc, None, allowed_only)
        after = None
        while True:
            ids, vals, total = self.select_ordered(pred, int(page), desc=desc, after=after, allowed_only=allowed_only)
            if ids.size:
                yield ids, vals
            if total <= ids.size:
                return
            after = (int(vals[-1]), int(ids[-1]))

    # -- row aggregation
    @classmethod
    def _agg_args(cls, by, width, limit, by_count, allowed_only):
        """The checked arguments of aggregate_where -> (by, width, limit, flags); limit stays None when it is None."""
        if not isinstance(by_count, (bool, np.bool_)):
            raise TypeError(f"by_count must be a bool, got {type(by_count).__name__}")
        flags = cls._rowpred_flags(allowed_only) | (AGG_ORDER_COUNT if by_count else 0)
        if not isinstance(by, (int, np.integer)) or isinstance(by, (bool, np.bool_)):
            raise TypeError(f"by must be AGG_BY_LABEL, AGG_BY_VALUE or AGG_BY_TAG, got {type(by).__name__}")
        if int(by) not in (AGG_BY_LABEL, AGG_BY_VALUE, AGG_BY_TAG):
            raise ValueError(f"by must be AGG_BY_LABEL, AGG_BY_VALUE or AGG_BY_TAG, got {by}")
        if width is not None:
            if not isinstance(width, (int, np.integer)) or isinstance(width, (bool, np.bool_)):
                raise TypeError(f"width must be an int, got {type(width).__name__}")
            if not 1 <= int(width) < (1 << 63):
                raise ValueError(f"width must be in 1..2^63-1, got {width}")
        elif int(by) == AGG_BY_VALUE:
            raise ValueError("AGG_BY_VALUE needs a width")
        if limit is not None:
            if not isinstance(limit, (int, np.integer)) or isinstance(limit, (bool, np.bool_)):
                raise TypeError(f"limit must be an int or None, got {type(limit).__name__}")
            if not 0 <= int(limit) < (1 << 32):
                raise ValueError(f"limit must fit 32 unsigned bits, got {limit}")
            limit = int(limit)
        return int(by), int(width) if width is not None and int(by) == AGG_BY_VALUE else 0, limit, flags

    def aggregate_where(self, pred, by: int, width=None, limit=None, by_count: bool = False, allowed_only: bool = False):
        """The rows in scope matching one predicate, grouped by label (AGG_BY_LABEL), by floor(value / width)
        (AGG_BY_VALUE) or by every tag bit a row has set (AGG_BY_TAG) -> (groups [n] of AGG_GROUP_DTYPE, n_groups, n_rows):
        per group its key, row count, min / max / wrapping sum of the values and smallest id, by key ascending or
        (by_count) by count descending, then key (vrod_index_aggregate_where).  n_groups is exact whatever the limit,
        n_rows the rows considered.  limit=None asks for the number of groups first and then for all of them; limit=0
        only counts.  More than MAX_AGG_GROUPS groups raise VrodError with code ERR_CAPACITY."""
        p = self._row_preds(pred, 1)
        by, width, limit, flags = self._agg_args(by, width, limit, by_count, allowed_only)
        n, groups, rows = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if limit is None:
            check(self._L.vrod_index_aggregate_where(self._h, _ptr(p), flags, by, width, 0, C.byref(n), C.byref(groups), C.byref(rows), None))
            limit = groups.value
        out = np.empty(max(min(limit, MAX_AGG_GROUPS), 1), AGG_GROUP_DTYPE)
        check(self._L.vrod_index_aggregate_where(self._h, _ptr(p), flags, by, width, limit, C.byref(n), C.byref(groups), C.byref(rows),
                                                 _ptr(out) if limit else None))
        return out[:n.value], groups.value, rows.value

    # -- group centroids
    def centroids_where(self, pred, by: int, width=None, capacity=None, sums: bool = False, allowed_only: bool = False, out=None):
        """The rows in scope matching one predicate, grouped by label (AGG_BY_LABEL) or by floor(value / width)
        (AGG_BY_VALUE) -> (groups [n] of CENTROID_GROUP_DTYPE, vectors [n, dim] float32): per group its key, row count and
        smallest id as aggregate_where reports them, by key ascending, and the exact mean (sums: the sum) of its rows as
        get_rows reads them (vrod_index_centroids_where): an integer sum of quantised elements, so no bit depends on the
        order of the rows.  capacity=None sizes itself with aggregate_where(limit=0); more groups than `capacity` raise
        VrodError with code ERR_CAPACITY.  `out`: a CUDA float32 tensor [>= capacity, dim] (a strided view is fine) makes
        this the device form, and the vectors returned are its first n rows."""
        p = self._row_preds(pred, 1)
        if not isinstance(sums, (bool, np.bool_)):
            raise TypeError(f"sums must be a bool, got {type(sums).__name__}")
        if isinstance(by, (int, np.integer)) and not isinstance(by, (bool, np.bool_)) and int(by) == AGG_BY_TAG:
            raise ValueError("by must be AGG_BY_LABEL or AGG_BY_VALUE: a row can carry several tags")
        by, width, _, flags = self._agg_args(by, width, None, False, allowed_only)
        flags |= CENTROID_SUM if sums else 0
        if capacity is not None:
            if not isinstance(capacity, (int, np.integer)) or isinstance(capacity, (bool, np.bool_)):
                raise TypeError(f"capacity must be an int or None, got {type(capacity).__name__}")
            if not 1 <= int(capacity) <= MAX_CENTROID_GROUPS:
                raise ValueError(f"capacity must be in 1..{MAX_CENTROID_GROUPS}, got {capacity}")
            capacity = int(capacity)
        if out is not None:
            rows, src, stride, stream = self._device_rows(out, "out")
            if src != SRC_F32:
                raise ValueError(f"out must be a float32 tensor [capacity, {self.dim}]")
        if capacity is None:
            capacity = min(max(self.aggregate_where(p, by, width=width or None, limit=0, allowed_only=allowed_only)[1], 1), MAX_CENTROID_GROUPS)
            if out is not None:
                capacity = max(min(capacity, rows), 1)
        if out is not None and rows < capacity:
            raise ValueError(f"out must hold {capacity} rows, got {rows}")
        groups = np.empty(capacity, CENTROID_GROUP_DTYPE)
        n, n_rows = C.c_uint64(), C.c_uint64()
        if out is not None:
            check(self._L.vrod_index_centroids_where_device(self._h, _ptr(p), flags, by, width, capacity, C.byref(n), C.byref(n_rows), _ptr(groups),
                                                            out.data_ptr(), stride, stream))
            return groups[:n.value], out[:n.value]
        vectors = np.empty((capacity, self.dim), np.float32)
        check(self._L.vrod_index_centroids_where(self._h, _ptr(p), flags, by, width, capacity, C.byref(n), C.byref(n_rows), _ptr(groups), _ptr(vectors),
                                                 self.dim))
        return groups[:n.value], vectors[:n.value]

    # -- duplicate rows
    @staticmethod
    def _dup_flags(within_label, narrow_hash=False) -> int:
        for name, v in (("within_label", within_label), ("narrow_hash", narrow_hash)):
            if not isinstance(v, (bool, np.bool_)):
                raise TypeError(f"{name} must be a bool, got {type(v).__name__}")
        return (DUP_WITHIN_LABEL if within_label else 0) | (DUP_NARROW_HASH if narrow_hash else 0)

    def find_duplicates(self, within_label: bool = False, narrow_hash: bool = False, stats: bool = False):
        """uint64 [count]: entry i = the smallest id among the live rows whose stored bits equal row i's (its own id when it
        has no copy), ID_NONE for a deleted row (vrod_index_find_duplicates).  within_label: equal rows with different
        labels are not duplicates.  narrow_hash: a diagnostic, the same result through an 8-bit hash.  stats=True:
        -> (map, dict of vrod_dup_stats)."""
        flags = self._dup_flags(within_label, narrow_hash)
        n = self.count
        out = np.empty(max(n, 1), dtype=np.uint64)
        st = DupStats()
        check(self._L.vrod_index_find_duplicates(self._h, flags, _ptr(out) if n else None, n, C.byref(st)))
        return (out[:n], st.as_dict()) if stats else out[:n]

    def find_duplicates_device(self, within_label: bool = False, narrow_hash: bool = False, out_first=None):
        """find_duplicates into a CUDA int64 tensor [count] (the bits of uint64), complete on return -> (map, stats dict)
        (vrod_index_find_duplicates_device)."""
        import torch
        flags = self._dup_flags(within_label, narrow_hash)
        n = self.count
        dev = torch.device("cuda", self.device)
        out_first = _device_out(out_first, max(n, 1), torch.int64, dev)
        n_out, stream = self._device_u64(out_first, "out_first")
        if n_out < n:
            raise ValueError(f"out_first must hold {n} ids")
        st = DupStats()
        check(self._L.vrod_index_find_duplicates_device(self._h, flags, out_first.data_ptr() if n else None, n, C.byref(st), stream))
        return out_first, st.as_dict()

    def delete_duplicates(self, within_label: bool = False) -> int:
        """Delete every live row that is not the smallest id of its class, as delete() of those ids
        (vrod_index_delete_duplicates).  -> rows that died."""
        flags = self._dup_flags(within_label)
        out = C.c_uint64()
        check(self._L.vrod_index_delete_duplicates(self._h, flags, C.byref(out)))
        return out.value

    # -- row lookup
    @staticmethod
    def _rowfind_flags(narrow_hash=False, small_batch=False) -> int:
        for name, v in (("narrow_hash", narrow_hash), ("small_batch", small_batch)):
            if not isinstance(v, (bool, np.bool_)):
                raise TypeError(f"{name} must be a bool, got {type(v).__name__}")
        return (ROWFIND_NARROW_HASH if narrow_hash else 0) | (ROWFIND_SMALL_BATCH if small_batch else 0)

    def _rowfind_host(self, fn, rows, narrow_hash, small_batch, stats):
        flags = self._rowfind_flags(narrow_hash, small_batch)
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        n = rows.shape[0]
        out = np.empty(max(n, 1), dtype=np.uint64)
        st = RowfindStats()
        check(fn(self._h, _ptr(rows) if n else None, n, flags, _ptr(out) if n else None, C.byref(st)))
        return (out[:n], st.as_dict()) if stats else out[:n]

    def _rowfind_device(self, fn, t, narrow_hash, small_batch, out_ids):
        import torch
        flags = self._rowfind_flags(narrow_hash, small_batch)
        n, src, stride, stream = self._device_rows(t)
        out_ids = _device_out(out_ids, (max(n, 1),), torch.int64, t.device)
        n_out, _ = self._device_u64(out_ids, "out_ids")
        if n_out < n:
            raise ValueError(f"out_ids must hold {n} ids")
        st = RowfindStats()
        check(fn(self._h, t.data_ptr() if n else None, src, stride, n, flags, out_ids.data_ptr() if n else None, C.byref(st), stream))
        return out_ids, st.as_dict()

    def find_rows(self, rows: np.ndarray, narrow_hash: bool = False, small_batch: bool = False, stats: bool = False):
        """uint64 [n]: entry i = the smallest id among the live rows whose stored bits equal rows[i] as add() would store it,
        ID_NONE if there is none (vrod_index_find_rows).  The handle does not change.  narrow_hash, small_batch:
        diagnostics, the same result through an 8-bit hash / lookup batches of 96 rows.  stats=True: -> (ids, dict of
        vrod_rowfind_stats)."""
        return self._rowfind_host(self._L.vrod_index_find_rows, rows, narrow_hash, small_batch, stats)

    def find_rows_device(self, t, narrow_hash: bool = False, small_batch: bool = False, out_ids=None):
        """find_rows from a CUDA tensor [n, dim] (float32 / bfloat16 / float16, any row stride >= dim) into a CUDA int64
        tensor (the bits of uint64), complete on return -> (ids, stats dict) (vrod_index_find_rows_device)."""
        return self._rowfind_device(self._L.vrod_index_find_rows_device, t, narrow_hash, small_batch, out_ids)

    def add_unique(self, rows: np.ndarray, narrow_hash: bool = False, small_batch: bool = False, stats: bool = False):
        """An idempotent add(): rows[i] with a live stored copy gets that row's smallest id, a repeat of an earlier row of
        the call gets that row's id, every other row is appended as add() would append it (vrod_index_add_unique).
        -> each row's id, uint64 [n]; stats=True: -> (ids, dict of vrod_rowfind_stats)."""
        return self._rowfind_host(self._L.vrod_index_add_unique, rows, narrow_hash, small_batch, stats)

    def add_unique_device(self, t, narrow_hash: bool = False, small_batch: bool = False, out_ids=None):
        """add_unique from a CUDA tensor, the ids into a CUDA int64 tensor -> (ids, stats dict)
        (vrod_index_add_unique_device)."""
        return self._rowfind_device(self._L.vrod_index_add_unique_device, t, narrow_hash, small_batch, out_ids)

    # -- near-duplicate rows
    @staticmethod
    def _near_args(threshold, small_pool=False):
        if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)):
            raise TypeError(f"threshold must be a number, got {type(threshold).__name__}")
        if not isinstance(small_pool, (bool, np.bool_)):
            raise TypeError(f"small_pool must be a bool, got {type(small_pool).__name__}")
        return float(np.float32(threshold)), NEAR_SMALL_POOL if small_pool else 0

    def find_near_duplicates(self, threshold, small_pool: bool = False, stats: bool = False):
        """uint64 [count]: entry i = the smallest id of row i's class -- the connected component, among the eligible rows
        (live, allowed by the filter), of the graph that joins two rows when one's stored form scores the other at least as
        well as `threshold` (single linkage: a~b and b~c put a and c in one class) -- its own id when no row qualifies,
        ID_NONE for a row that is not eligible (vrod_index_find_near_duplicates).  small_pool: a diagnostic, the same
        result through a hit pool that makes batches split.  stats=True: -> (map, dict of vrod_near_stats)."""
        thr, flags = self._near_args(threshold, small_pool)
        n = self.count
        out = np.empty(max(n, 1), dtype=np.uint64)
        st = NearStats()
        check(self._L.vrod_index_find_near_duplicates(self._h, thr, flags, _ptr(out) if n else None, n, C.byref(st)))
        return (out[:n], st.as_dict()) if stats else out[:n]

    def find_near_duplicates_device(self, threshold, small_pool: bool = False, out_first=None):
        """find_near_duplicates into a CUDA int64 tensor [count] (the bits of uint64), complete on return -> (map, stats
        dict) (vrod_index_find_near_duplicates_device)."""
        import torch
        thr, flags = self._near_args(threshold, small_pool)
        n = self.count
        dev = torch.device("cuda", self.device)
        out_first = _device_out(out_first, max(n, 1), torch.int64, dev)
        n_out, stream = self._device_u64(out_first, "out_first")
        if n_out < n:
            raise ValueError(f"out_first must hold {n} ids")
        st = NearStats()
        check(self._L.vrod_index_find_near_duplicates_device(self._h, thr, flags, out_first.data_ptr() if n else None, n, C.byref(st), stream))
        return out_first, st.as_dict()

    def delete_near_duplicates(self, threshold) -> int:
        """Delete every eligible row that is not the smallest id of its class, as delete() of those ids
        (vrod_index_delete_near_duplicates).  -> rows that died."""
        thr, flags = self._near_args(threshold)
        out = C.c_uint64()
        check(self._L.vrod_index_delete_near_duplicates(self._h, thr, flags, C.byref(out)))
        return out.value

    def set_id_offset(self, off: int):
        check(self._L.vrod_index_set_id_offset(self._h, int(off)))
        self._id_offset = int(off)

    def get_rows(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), dtype=np.float32)
        check(self._L.vrod_index_get_rows(self._h, int(first), int(n), _ptr(out)))
        return out

    # -- knobs
    def set_path(self, path: int):
        check(self._L.vrod_index_set_path(self._h, int(path)))

    def set_profiling(self, level):
        """0/False: off; 1/True: scan_ms (events attached to the scan dispatches); 2: + total_ms."""
        check(self._L.vrod_index_set_profiling(self._h, int(level)))

    def last_stats(self) -> dict:
        st = SearchStats()
        check(self._L.vrod_index_last_stats(self._h, C.byref(st)))
        return st.as_dict()

    def shard_stats(self, shard: int) -> dict:
        """Counters of one shard of the last completed search + the device it lives on."""
        st = SearchStats()
        dev = C.c_int32(-1)
        check(self._L.vrod_index_shard_stats(self._h, int(shard), C.byref(dev), C.byref(st)))
        d = st.as_dict()
        d["device"] = dev.value
        return d

    # -- search
    def _queries(self, queries) -> np.ndarray:
        """Any [nq, dim] (or [dim]) array-like -> a contiguous [nq, dim] fp32 array."""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim == 1:
            queries = queries[None, :]
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}]")
        return queries

    def _device_queries(self, t, what="queries"):
        """Checks a device tensor of queries ([n, dim] fp32, contiguous) -> (n, its device, its device's current stream)."""
        import torch
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError(f"{what} must be [n, {self.dim}]")
        return t.shape[0], t.device, C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def search(self, queries: np.ndarray, k: int):
        """numpy [nq, dim] fp32 -> (ids uint64 [nq, k], scores float32 [nq, k])."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        ids, sc = _out(nq, k, np.uint64, np.float32)
        check(self._L.vrod_search(self._h, _ptr(queries), nq, int(k), _ptr(ids), _ptr(sc)))
        return ids, sc

    def search_labeled(self, queries: np.ndarray, k: int, labels):
        """search() with a label per query (vrod_search_labeled): query q sees only the eligible rows that carry labels[q].
        numpy [nq, dim] fp32, nq integer labels -> (ids uint64 [nq, k], scores float32 [nq, k])."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        lab = self._labels(labels, nq)
        ids, sc = _out(nq, k, np.uint64, np.float32)
        check(self._L.vrod_search_labeled(self._h, _ptr(queries), nq, int(k), _ptr(lab), _ptr(ids), _ptr(sc)))
        return ids, sc

    def search_labeled_device(self, d_queries, k: int, d_labels, out_ids=None, out_scores=None):
        """torch CUDA tensors: queries [nq, dim] fp32, labels [nq] int32 (the bits of uint32) -> (ids int64-viewed-uint64
        [nq, k], scores [nq, k]) on the device, complete on return."""
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        if d_labels.dtype != torch.int32:
            raise TypeError(f"labels must be an int32 tensor, got {d_labels.dtype}")
        if d_labels.numel() != nq:
            raise ValueError(f"labels must hold {nq} values, got {d_labels.numel()}")
        assert d_labels.is_cuda and d_labels.is_contiguous()
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        check(self._L.vrod_search_labeled_device(self._h, d_queries.data_ptr(), nq, int(k), d_labels.data_ptr(), out_ids.data_ptr(),
                                                 out_scores.data_ptr(), stream))
        return out_ids, out_scores

    def search_tagged(self, queries: np.ndarray, k: int, preds):
        """search() with a tag predicate per query (vrod_search_tagged): preds is [nq, 3] uint64, the columns any, all,
        none; query q sees only the eligible rows whose tags t satisfy (any == 0 or t & any) and t & all == all and not
        t & none.  numpy [nq, dim] fp32 -> (ids uint64 [nq, k], scores float32 [nq, k])."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        p = self._u64(preds, "preds", (nq, 3))
        ids, sc = _out(nq, k, np.uint64, np.float32)
        check(self._L.vrod_search_tagged(self._h, _ptr(queries), nq, int(k), _ptr(p), _ptr(ids), _ptr(sc)))
        return ids, sc

    def search_tagged_device(self, d_queries, k: int, d_preds, out_ids=None, out_scores=None):
        """torch CUDA tensors: queries [nq, dim] fp32, preds [nq, 3] int64 (the bits of uint64: any, all, none) -> (ids
        int64-viewed-uint64 [nq, k], scores [nq, k]) on the device, complete on return."""
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        if d_preds.dtype != torch.int64:
            raise TypeError(f"preds must be an int64 tensor, got {d_preds.dtype}")
        if tuple(d_preds.shape) != (nq, 3):
            raise ValueError(f"preds must be [{nq}, 3], got {tuple(d_preds.shape)}")
        assert d_preds.is_cuda and d_preds.is_contiguous()
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        check(self._L.vrod_search_tagged_device(self._h, d_queries.data_ptr(), nq, int(k), d_preds.data_ptr(), out_ids.data_ptr(),
                                                out_scores.data_ptr(), stream))
        return out_ids, out_scores

    def search_where(self, queries: np.ndarray, k: int, preds):
        """search() with a tags + value-interval predicate per query (vrod_search_where): preds is a structured array of
        WHERE_DTYPE or [nq, 5] integers, the columns any, all, none, lo, hi; query q sees only the eligible rows whose tags
        satisfy (any, all, none) as in search_tagged and whose value v satisfies lo <= v <= hi (signed, inclusive).
        numpy [nq, dim] fp32 -> (ids uint64 [nq, k], scores float32 [nq, k])."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        p = self._where(preds, nq)
        ids, sc = _out(nq, k, np.uint64, np.float32)
        check(self._L.vrod_search_where(self._h, _ptr(queries), nq, int(k), _ptr(p), _ptr(ids), _ptr(sc)))
        return ids, sc

    def search_where_device(self, d_queries, k: int, d_preds, out_ids=None, out_scores=None):
        """torch CUDA tensors: queries [nq, dim] fp32, preds [nq, 5] int64 (any, all, none as the bits of uint64; lo, hi)
        -> (ids int64-viewed-uint64 [nq, k], scores [nq, k]) on the device, complete on return."""
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        if d_preds.dtype != torch.int64:
            raise TypeError(f"preds must be an int64 tensor, got {d_preds.dtype}")
        if tuple(d_preds.shape) != (nq, 5):
            raise ValueError(f"preds must be [{nq}, 5], got {tuple(d_preds.shape)}")
        assert d_preds.is_cuda and d_preds.is_contiguous()
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        check(self._L.vrod_search_where_device(self._h, d_queries.data_ptr(), nq, int(k), d_preds.data_ptr(), out_ids.data_ptr(),
                                               out_scores.data_ptr(), stream))
        return out_ids, out_scores

    def search_grouped(self, queries: np.ndarray, k: int):
        """The best row of each label, the k best labels per query (vrod_search_grouped): numpy [nq, dim] fp32 ->
        (ids uint64 [nq, k], scores float32 [nq, k], labels uint32 [nq, k]); slots beyond the distinct labels of the
        eligible rows are (ID_NONE, NaN, 0)."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        ids, sc, lab = _out(nq, k, np.uint64, np.float32, np.uint32)
        check(self._L.vrod_search_grouped(self._h, _ptr(queries), nq, int(k), _ptr(ids), _ptr(sc), _ptr(lab)))
        return ids, sc, lab

    def search_grouped_device(self, d_queries, k: int, out_ids=None, out_scores=None, out_labels=None, want_labels=True):
        """torch CUDA tensor [nq, dim] fp32 -> (ids int64-viewed-uint64 [nq, k], scores [nq, k], labels int32-viewed-uint32
        [nq, k]) on the device, complete on return.  want_labels=False passes no label buffer (labels is None)."""
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        if want_labels:
            out_labels = _device_out(out_labels, (nq, k), torch.int32, dev)
        check(self._L.vrod_search_grouped_device(self._h, d_queries.data_ptr(), nq, int(k), out_ids.data_ptr(), out_scores.data_ptr(),
                                                 out_labels.data_ptr() if out_labels is not None else None, stream))
        return out_ids, out_scores, out_labels

    # -- multi-vector search: a query is a set of vectors, a document the rows of one label, scored by MaxSim
    def _multivec_args(self, vectors, lims):
        """A list of [m_i, dim] arrays, or (vectors [n, dim], lims [nq + 1]) -> contiguous fp32 vectors and uint32 lims."""
        if lims is None:
            parts = [np.asarray(v, dtype=np.float32) for v in vectors]
            parts = [v[None, :] if v.ndim == 1 else v for v in parts]
            for v in parts:
                if v.ndim != 2 or v.shape[1] != self.dim:
                    raise ValueError(f"every query must be [m, {self.dim}]")
            lims = np.cumsum([0] + [v.shape[0] for v in parts])
            vectors = np.concatenate(parts) if parts else np.zeros((0, self.dim), np.float32)
        vectors = np.ascontiguousarray(vectors, dtype=np.float32)
        if vectors.ndim != 2 or vectors.shape[1] != self.dim:
            raise ValueError(f"vectors must be [n, {self.dim}]")
        la = np.asarray(lims)
        if la.ndim != 1 or la.size < 1 or la.dtype.kind not in "iu":
            raise ValueError("lims must be a vector of nq + 1 integers")
        if la.size and (int(la.min()) < 0 or int(la.max()) > 0xFFFFFFFF):
            raise ValueError("lims must fit uint32")
        la = np.ascontiguousarray(la, dtype=np.uint32)
        if int(la[-1]) != vectors.shape[0]:
            raise ValueError(f"lims[-1] = {int(la[-1])} must equal the number of vectors, {vectors.shape[0]}")
        return vectors, la

    def search_multivec(self, vectors, k: int, lims=None):
        """The k best documents (labels) per multi-vector query (vrod_search_multivec).  `vectors`: a list of [m_i, dim]
        arrays, one per query, or -- with lims [nq + 1] -- all vectors as [n, dim], query q owning rows lims[q]:lims[q + 1].
        -> (labels uint32 [nq, k], scores float32 [nq, k], found uint32 [nq]); slots past found[q] are (0, NaN)."""
        vectors, la = self._multivec_args(vectors, lims)
        nq = la.size - 1
        lab, sc = _out(nq, k, np.uint32, np.float32)
        found = np.empty(nq, dtype=np.uint32)
        check(self._L.vrod_search_multivec(self._h, _ptr(vectors), _ptr(la), nq, int(k), _ptr(lab), _ptr(sc), _ptr(found)))
        return lab, sc, found

    def search_multivec_device(self, d_vectors, d_lims, k: int, out_labels=None, out_scores=None, out_found=None, want_found=True):
        """torch CUDA tensors: vectors [n, dim] fp32, lims [nq + 1] int32 (the bits of uint32) -> (labels int32-viewed-uint32
        [nq, k], scores [nq, k], found int32 [nq]) on the device, complete on return.  want_found=False passes no found
        buffer (found is None)."""
        import torch
        _, dev, stream = self._device_queries(d_vectors, "vectors")
        if d_lims.dtype != torch.int32:
            raise TypeError(f"lims must be an int32 tensor, got {d_lims.dtype}")
        if d_lims.dim() != 1 or d_lims.numel() < 1:
            raise ValueError("lims must be a vector of nq + 1 entries")
        assert d_lims.is_cuda and d_lims.is_contiguous()
        nq = d_lims.numel() - 1
        out_labels = _device_out(out_labels, (nq, k), torch.int32, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        if want_found:
            out_found = _device_out(out_found, (nq,), torch.int32, dev)
        check(self._L.vrod_search_multivec_device(self._h, d_vectors.data_ptr(), d_lims.data_ptr(), nq, int(k), out_labels.data_ptr(),
                                                  out_scores.data_ptr(), out_found.data_ptr() if out_found is not None else None, stream))
        return out_labels, out_scores, out_found

    def last_multivec(self) -> dict:
        """What the last search_multivec call did (vrod_index_last_multivec): which route answered how many queries."""
        st = MultivecStats()
        check(self._L.vrod_index_last_multivec(self._h, C.byref(st)))
        return st.as_dict()

    # -- diversified search: exact greedy MMR over the certified top pool
    def search_diverse(self, queries: np.ndarray, k: int, pool: int, lam: float):
        """k rows of the `pool` best per query, picked greedily by lam * relevance - (1 - lam) * similarity to the rows
        already picked (vrod_search_diverse): numpy [nq, dim] fp32 -> (ids uint64 [nq, k], scores float32 [nq, k], mmr
        float32 [nq, k]) in selection order; slots past the eligible rows are (ID_NONE, NaN, NaN)."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        ids, sc, mmr = _out(nq, k, np.uint64, np.float32, np.float32)
        check(self._L.vrod_search_diverse(self._h, _ptr(queries), nq, int(k), int(pool), float(lam), _ptr(ids), _ptr(sc), _ptr(mmr)))
        return ids, sc, mmr

    def search_diverse_device(self, d_queries, k: int, pool: int, lam: float, out_ids=None, out_scores=None, out_mmr=None, want_mmr=True):
        """torch CUDA tensor [nq, dim] fp32 -> (ids int64-viewed-uint64 [nq, k], scores [nq, k], mmr [nq, k]) on the device,
        complete on return.  want_mmr=False passes no mmr buffer (mmr is None)."""
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        if want_mmr:
            out_mmr = _device_out(out_mmr, (nq, k), torch.float32, dev)
        check(self._L.vrod_search_diverse_device(self._h, d_queries.data_ptr(), nq, int(k), int(pool), float(lam), out_ids.data_ptr(),
                                                 out_scores.data_ptr(), out_mmr.data_ptr() if out_mmr is not None else None, stream))
        return out_ids, out_scores, out_mmr

    # -- search by stored row: the queries are rows the handle already holds, used as stored
    @classmethod
    def _query_ids(cls, ids) -> np.ndarray:
        """Ids as searches report them: any integer array-like without a negative value -> a contiguous uint64 vector."""
        a = np.asarray(ids)
        if a.size and a.dtype.kind == "i" and int(a.min()) < 0:
            raise ValueError("ids must not be negative")
        if a.dtype.kind == "b":
            raise TypeError("ids must be integers, got bool")
        return cls._ids(ids)

    def search_by_ids(self, ids, k: int, exclude_self: bool = False):
        """Each stored row's nearest neighbours (vrod_search_by_ids): integer ids [nq] -> (ids uint64 [nq, k], scores
        float32 [nq, k]).  The query is the prepared row as stored.  exclude_self=True: the row itself is no candidate
        (k <= MAX_K - 1).  An id that is no live row raises VrodError (code 1)."""
        a = self._query_ids(ids)
        nq = a.size
        out_ids, sc = _out(nq, k, np.uint64, np.float32)
        check(self._L.vrod_search_by_ids(self._h, _ptr(a), nq, int(k), BYID_EXCLUDE_SELF if exclude_self else 0,
                                         _ptr(out_ids), _ptr(sc)))
        return out_ids, sc

    def search_by_ids_device(self, d_ids, k: int, exclude_self: bool = False, out_ids=None, out_scores=None):
        """torch CUDA tensor of ids [nq] int64 (the bits of uint64) -> (ids int64-viewed-uint64 [nq, k], scores [nq, k]) on
        the device, complete on return."""
        import torch
        if d_ids.dtype != torch.int64:
            raise TypeError(f"ids must be an int64 tensor, got {d_ids.dtype}")
        assert d_ids.is_cuda and d_ids.is_contiguous()
        nq = d_ids.numel()
        out_ids = _device_out(out_ids, (nq, k), torch.int64, d_ids.device)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, d_ids.device)
        stream = torch.cuda.current_stream(d_ids.device).cuda_stream
        check(self._L.vrod_search_by_ids_device(self._h, d_ids.data_ptr(), nq, int(k), BYID_EXCLUDE_SELF if exclude_self else 0,
                                                out_ids.data_ptr(), out_scores.data_ptr(), C.c_void_p(stream)))
        return out_ids, out_scores

    def knn_graph(self, k: int, first_id=None, n=None):
        """The exact k-NN graph (vrod_knn_graph): for the rows with ids first_id .. first_id + n - 1 (default: every row,
        from the smallest id a search on this handle reports) the k nearest other eligible rows -> (ids uint64 [n, k],
        scores float32 [n, k]); a deleted row's result row is all (ID_NONE, NaN).  The default range starts at the offset
        given to set_id_offset() of THIS object (0 if it was never called): the C ABI has no getter, so a handle whose
        offset was set any other way must pass first_id and n."""
        if first_id is None:
            if n is not None:
                raise ValueError("n needs first_id")
            first_id = self._first_id()
        first_id = int(first_id)
        if first_id < 0:
            raise ValueError("first_id must not be negative")
        if n is None:
            n = self._first_id() + self.count - first_id
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        out_ids, sc = _out(n, k, np.uint64, np.float32)
        check(self._L.vrod_knn_graph(self._h, first_id, n, int(k), _ptr(out_ids), _ptr(sc)))
        return out_ids, sc

    # -- search by weighted examples: the query is combined on the device from a vector and stored rows
    @classmethod
    def _ragged_ids(cls, ids, lims, what):
        """A list of per-query id sequences, or -- with lims [nq + 1] -- all ids flat -> (uint64 ids, uint32 lims)."""
        if lims is None:
            parts = [cls._query_ids(p) for p in ids]
            lims = np.cumsum([0] + [p.size for p in parts])
            flat = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
        else:
            flat = cls._query_ids(ids)
        la = np.asarray(lims)
        if la.ndim != 1 or la.size < 1 or la.dtype.kind not in "iu":
            raise ValueError(f"{what} lims must be a vector of nq + 1 integers")
        if int(la.min()) < 0 or int(la.max()) > 0xFFFFFFFF:
            raise ValueError(f"{what} lims must fit uint32")
        la = np.ascontiguousarray(la, dtype=np.uint32)
        if int(la[-1]) != flat.size:
            raise ValueError(f"{what} lims[-1] = {int(la[-1])} must equal the number of ids, {flat.size}")
        return np.ascontiguousarray(flat, dtype=np.uint64), la

    def search_combined(self, k: int, term_ids, term_weights, term_lims=None, vectors=None, vector_weights=None, exclude_ids=None,
                        exclude_lims=None, exclude_terms: bool = False):
        """Search by weighted examples (vrod_search_combined).  Query q is fl-summed in order from row q of `vectors` ([nq, dim]
        fp32 or None; prepared as a query, weight vector_weights[q] or 1) and the stored rows term_ids of q as stored, each
        times its weight; the result leaves out q's exclude_ids and, with exclude_terms, its terms.  term_ids / term_weights
        (and exclude_ids): a list of per-query sequences, or flat arrays with term_lims (exclude_lims) [nq + 1].
        -> (ids uint64 [nq, k], scores float32 [nq, k])."""
        tid, tl = self._ragged_ids(term_ids, term_lims, "term")
        nq = tl.size - 1
        if term_lims is None:
            tw = np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in term_weights]) if nq else np.zeros(0, np.float32)
        else:
            tw = np.asarray(term_weights, dtype=np.float32).reshape(-1)
        tw = np.ascontiguousarray(tw, dtype=np.float32)
        if tw.size != tid.size:
            raise ValueError(f"term_weights must hold {tid.size} values, got {tw.size}")
        vec = vw = None
        if vectors is not None:
            vec = self._queries(vectors)
            if vec.shape[0] != nq:
                raise ValueError(f"vectors must be [{nq}, {self.dim}]")
            if vector_weights is not None:
                vw = np.ascontiguousarray(np.asarray(vector_weights, dtype=np.float32).reshape(-1))
                if vw.size != nq:
                    raise ValueError(f"vector_weights must hold {nq} values, got {vw.size}")
        xid = xl = None
        if exclude_ids is not None:
            xid, xl = self._ragged_ids(exclude_ids, exclude_lims, "exclude")
            if xl.size != nq + 1:
                raise ValueError(f"exclude lists for {xl.size - 1} queries, terms for {nq}")
        out_ids, sc = _out(nq, k, np.uint64, np.float32)
        check(self._L.vrod_search_combined(self._h, _ptr(vec), _ptr(vw), _ptr(tl), _ptr(tid), _ptr(tw), _ptr(xl), _ptr(xid), nq, int(k),
                                           COMBINED_EXCLUDE_TERMS if exclude_terms else 0, _ptr(out_ids), _ptr(sc)))
        return out_ids, sc

    def search_combined_device(self, k: int, d_term_lims, d_term_ids, d_term_weights, d_vectors=None, d_vector_weights=None,
                               d_exclude_lims=None, d_exclude_ids=None, exclude_terms: bool = False, out_ids=None, out_scores=None):
        """torch CUDA tensors: term_lims [nq + 1] int32 (the bits of uint32), term_ids int64 (the bits of uint64), term_weights
        fp32; optional vectors [nq, dim] fp32, vector_weights [nq] fp32, exclude_lims [nq + 1] int32, exclude_ids int64 ->
        (ids int64-viewed-uint64 [nq, k], scores [nq, k]) on the device, complete on return."""
        import torch

        def ptr(t, dtype, what):
            if t is None:
                return None
            if t.dtype != dtype:
                raise TypeError(f"{what} must be a {dtype} tensor, got {t.dtype}")
            assert t.is_cuda and t.is_contiguous()
            return t.data_ptr()
        if d_term_lims.dim() != 1 or d_term_lims.numel() < 1:
            raise ValueError("term_lims must be a vector of nq + 1 entries")
        nq = d_term_lims.numel() - 1
        dev = d_term_lims.device
        if d_vectors is not None and self._device_queries(d_vectors, "vectors")[0] != nq:
            raise ValueError(f"vectors must be [{nq}, {self.dim}]")
        if d_exclude_lims is not None and d_exclude_lims.numel() != nq + 1:
            raise ValueError(f"exclude_lims must hold {nq + 1} entries")
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(self._L.vrod_search_combined_device(
            self._h, ptr(d_vectors, torch.float32, "vectors"), ptr(d_vector_weights, torch.float32, "vector_weights"),
            ptr(d_term_lims, torch.int32, "term_lims"), ptr(d_term_ids, torch.int64, "term_ids"),
            ptr(d_term_weights, torch.float32, "term_weights"), ptr(d_exclude_lims, torch.int32, "exclude_lims"),
            ptr(d_exclude_ids, torch.int64, "exclude_ids"), nq, int(k), COMBINED_EXCLUDE_TERMS if exclude_terms else 0,
            out_ids.data_ptr(), out_scores.data_ptr(), C.c_void_p(stream)))
        return out_ids, out_scores

    # -- candidate lists: every query is scored against the rows its own list of ids names
    def _candidate_args(self, queries, cand_ids, cand_lims):
        queries = self._queries(queries)
        cid, cl = self._ragged_ids(cand_ids, cand_lims, "candidate")
        if cl.size != queries.shape[0] + 1:
            raise ValueError(f"candidate lists for {cl.size - 1} queries, {queries.shape[0]} queries")
        return queries, cid, cl

    def search_candidates(self, queries: np.ndarray, k: int, cand_ids, cand_lims=None):
        """search() over a list of candidate ids per query (vrod_search_candidates): query q sees only the distinct ids of
        its list that are live, allowed rows, in any order; ids that are not are ignored.  cand_ids: a list of per-query
        sequences, or flat with cand_lims [nq + 1].  -> (ids uint64 [nq, k], scores float32 [nq, k])."""
        queries, cid, cl = self._candidate_args(queries, cand_ids, cand_lims)
        nq = queries.shape[0]
        ids, sc = _out(nq, k, np.uint64, np.float32)
        check(self._L.vrod_search_candidates(self._h, _ptr(queries), nq, int(k), _ptr(cl), _ptr(cid), _ptr(ids), _ptr(sc)))
        return ids, sc

    def score_candidates(self, queries: np.ndarray, cand_ids, cand_lims=None):
        """The canonical score of every listed id against its query (vrod_score_candidates), in the caller's order: NaN where
        the id is not a live, allowed row.  cand_ids as for search_candidates.  -> scores float32, flat, aligned with the
        ids (query q owns [lims[q], lims[q + 1]))."""
        queries, cid, cl = self._candidate_args(queries, cand_ids, cand_lims)
        sc = np.empty(cid.size, np.float32)
        check(self._L.vrod_score_candidates(self._h, _ptr(queries), queries.shape[0], _ptr(cl), _ptr(cid), _ptr(sc)))
        return sc

    def _device_candidates(self, d_queries, d_cand_lims, d_cand_ids):
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        if d_cand_lims.dtype != torch.int32:
            raise TypeError(f"cand_lims must be an int32 tensor, got {d_cand_lims.dtype}")
        if d_cand_ids.dtype != torch.int64:
            raise TypeError(f"cand_ids must be an int64 tensor, got {d_cand_ids.dtype}")
        if d_cand_lims.dim() != 1 or d_cand_lims.numel() != nq + 1:
            raise ValueError(f"cand_lims must hold {nq + 1} entries")
        assert d_cand_lims.is_cuda and d_cand_lims.is_contiguous() and d_cand_ids.is_cuda and d_cand_ids.is_contiguous()
        return nq, dev, stream

    def search_candidates_device(self, d_queries, k: int, d_cand_lims, d_cand_ids, out_ids=None, out_scores=None):
        """torch CUDA tensors: queries [nq, dim] fp32, cand_lims [nq + 1] int32 (the bits of uint32), cand_ids int64 (the bits
        of uint64) -> (ids int64-viewed-uint64 [nq, k], scores [nq, k]) on the device, complete on return."""
        import torch
        nq, dev, stream = self._device_candidates(d_queries, d_cand_lims, d_cand_ids)
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        check(self._L.vrod_search_candidates_device(self._h, d_queries.data_ptr(), nq, int(k), d_cand_lims.data_ptr(), d_cand_ids.data_ptr(),
                                                    out_ids.data_ptr(), out_scores.data_ptr(), stream))
        return out_ids, out_scores

    def score_candidates_device(self, d_queries, d_cand_lims, d_cand_ids, out_scores=None):
        """torch CUDA tensors as for search_candidates_device -> scores fp32, one per entry of cand_ids, on the device,
        complete on return."""
        import torch
        nq, dev, stream = self._device_candidates(d_queries, d_cand_lims, d_cand_ids)
        out_scores = _device_out(out_scores, (d_cand_ids.numel(),), torch.float32, dev)
        check(self._L.vrod_score_candidates_device(self._h, d_queries.data_ptr(), nq, d_cand_lims.data_ptr(), d_cand_ids.data_ptr(),
                                                   out_scores.data_ptr(), stream))
        return out_scores

    def _first_id(self) -> int:
        return getattr(self, "_id_offset", 0)

    def search_device(self, d_queries, k: int, out_ids=None, out_scores=None):
        """torch CUDA tensor [nq, dim] fp32 -> (ids int64-viewed-uint64 [nq,k], scores [nq,k]) on device."""
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        out_ids = _device_out(out_ids, (nq, k), torch.int64, dev)
        out_scores = _device_out(out_scores, (nq, k), torch.float32, dev)
        check(self._L.vrod_search_device(self._h, d_queries.data_ptr(), nq, int(k), out_ids.data_ptr(), out_scores.data_ptr(), stream))
        return out_ids, out_scores

    def search_synthetic_device(self, seed: int, first_row: int, nq: int, k: int, out_ids, out_scores):
        """Queries = rows [first_row, first_row+nq) of synthetic stream `seed`, generated on device."""
        import torch
        stream = torch.cuda.current_stream(out_ids.device).cuda_stream
        check(self._L.vrod_search_synthetic_device(self._h, int(seed), int(first_row), int(nq), int(k),
                                                   out_ids.data_ptr(), out_scores.data_ptr(), C.c_void_p(stream)))
        return out_ids, out_scores

    # -- range search: every row at least as good as a per-query threshold
    def _range_args(self, nq: int, threshold):
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(threshold, dtype=np.float32), (nq,)) if np.ndim(threshold) == 0
                                   else np.asarray(threshold, dtype=np.float32).reshape(-1))
        if thr.size != nq:
            raise ValueError(f"threshold must be a scalar or {nq} values, got {thr.size}")
        if np.isnan(thr).any():
            raise ValueError("threshold is NaN")
        return thr

    def range_search(self, queries: np.ndarray, threshold, capacity=None):
        """numpy [nq, dim] fp32 and a threshold (a scalar or nq values, in the units of the handle's scores) ->
        (lims uint64 [nq + 1], ids uint64 [lims[-1]], scores float32 [lims[-1]]): query q's rows are entries
        lims[q]:lims[q + 1], best first, every row whose score is >= (cosine, ip) / <= (l2) the threshold.
        capacity=None: a count-only call sizes the buffers; else a result larger than `capacity` raises VrodError with
        code ERR_CAPACITY (and .lims holds the exact counts)."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        thr = self._range_args(nq, threshold)
        lims = np.zeros(nq + 1, dtype=np.uint64)

        def call(cap, ids, sc):
            return self._L.vrod_range_search(self._h, _ptr(queries), nq, _ptr(thr), cap, _ptr(lims), _ptr(ids), _ptr(sc))
        if capacity is None:
            rc = call(0, None, None)
            if rc not in (0, _lib.ERR_CAPACITY):
                check(rc)
            capacity = int(lims[-1])
            if rc == 0:
                return lims, np.empty(0, np.uint64), np.empty(0, np.float32)
        capacity = int(capacity)
        ids = np.empty(max(capacity, 1), dtype=np.uint64)
        sc = np.empty(max(capacity, 1), dtype=np.float32)
        rc = call(capacity, ids if capacity else None, sc if capacity else None)
        if rc == _lib.ERR_CAPACITY:
            e = VrodError(rc, self._L.vrod_last_error().decode("utf-8", "replace"))
            e.lims = lims
            raise e
        check(rc)
        n = int(lims[-1])
        return lims, ids[:n], sc[:n]

    def range_search_device(self, d_queries, d_thresholds, capacity: int, out_lims=None, out_ids=None, out_scores=None):
        """torch CUDA tensors: queries [nq, dim] fp32, thresholds [nq] fp32 -> (rc, lims int64 [nq + 1], ids int64-viewed
        uint64 [capacity], scores [capacity]) on the device.  No retry: rc is 0 or ERR_CAPACITY (lims valid either way)."""
        import torch
        nq, dev, stream = self._device_queries(d_queries)
        assert d_thresholds.is_cuda and d_thresholds.dtype == torch.float32 and d_thresholds.is_contiguous()
        if d_thresholds.numel() != nq:
            raise ValueError(f"thresholds must hold {nq} values, got {d_thresholds.numel()}")
        out_lims = _device_out(out_lims, nq + 1, torch.int64, dev)
        out_ids = _device_out(out_ids, max(int(capacity), 1), torch.int64, dev)
        out_scores = _device_out(out_scores, max(int(capacity), 1), torch.float32, dev)
        rc = self._L.vrod_range_search_device(self._h, d_queries.data_ptr(), nq, d_thresholds.data_ptr(), int(capacity), out_lims.data_ptr(),
                                              out_ids.data_ptr() if capacity else None, out_scores.data_ptr() if capacity else None, stream)
        if rc not in (0, _lib.ERR_CAPACITY):
            check(rc)
        return rc, out_lims, out_ids, out_scores

    # -- pipelined search: begin(s+1) before end(s) keeps the device busy between batches
    def search_begin_device(self, d_queries, k: int, out_ids, out_scores):
        nq, _, stream = self._device_queries(d_queries)
        check(self._L.vrod_search_begin_device(self._h, d_queries.data_ptr(), nq, int(k), out_ids.data_ptr(), out_scores.data_ptr(), stream))

    def search_begin_synthetic_device(self, seed: int, first_row: int, nq: int, k: int, out_ids, out_scores):
        import torch
        stream = torch.cuda.current_stream(out_ids.device).cuda_stream
        check(self._L.vrod_search_begin_synthetic_device(self._h, int(seed), int(first_row), int(nq), int(k),
                                                         out_ids.data_ptr(), out_scores.data_ptr(), C.c_void_p(stream)))

    def search_end(self):
        """Complete the oldest pending search; its output tensors are final when this returns."""
        check(self._L.vrod_search_end(self._h))

    @property
    def pending(self) -> int:
        out = C.c_uint32()
        check(self._L.vrod_search_pending(self._h, C.byref(out)))
        return out.value


def snapshot_info(path) -> dict:
    """What a snapshot's header says (vrod_snapshot_info): host only, the header block alone is read."""
    out = SnapshotInfo()
    check(_lib.load().vrod_snapshot_info(os.fsencode(path), C.byref(out)))
    return out.as_dict()


def snapshot_verify(path) -> None:
    """Check a whole snapshot file on the host (vrod_snapshot_verify): raises VrodError if it is not sound."""
    check(_lib.load().vrod_snapshot_verify(os.fsencode(path)))


def merge_topk_device(device: int, metric, ids, scores, out_ids=None, out_scores=None):
    """ids/scores: torch CUDA tensors [n_lists, nq, k] (int64 bits of uint64 / float32) -> merged [nq, k]."""
    import torch
    L = _lib.load()
    n_lists, nq, k = ids.shape
    assert ids.is_contiguous() and scores.is_contiguous()
    out_ids = _device_out(out_ids, (nq, k), torch.int64, ids.device)
    out_scores = _device_out(out_scores, (nq, k), torch.float32, ids.device)
    stream = torch.cuda.current_stream(ids.device).cuda_stream
    check(L.vrod_merge_topk_device(int(device), _enum(metric, _METRICS, "metric"), ids.data_ptr(), scores.data_ptr(),
                                   n_lists, nq, k, out_ids.data_ptr(), out_scores.data_ptr(), C.c_void_p(stream)))
    return out_ids, out_scores


def merge_topk_packed_device(device: int, metric, packed, n_lists: int, nq: int, k: int, out_ids, out_scores):
    """packed: torch CUDA uint8 buffer of n_lists blocks (shard.alloc_packed layout) -> merged [nq, k]."""
    import torch
    L = _lib.load()
    assert packed.is_contiguous() and packed.numel() == n_lists * 12 * nq * k
    stream = torch.cuda.current_stream(packed.device).cuda_stream
    check(L.vrod_merge_topk_packed_device(int(device), _enum(metric, _METRICS, "metric"), packed.data_ptr(), n_lists, nq, k,
                                          out_ids.data_ptr(), out_scores.data_ptr(), C.c_void_p(stream)))
    return out_ids, out_scores


def synth_rows_device(device: int, seed: int, first_row: int, n: int, dim: int):
    """Synthetic rows generated on the device, returned as a torch tensor [n, dim]."""
    import torch
    L = _lib.load()
    out = torch.empty((n, dim), dtype=torch.float32, device=f"cuda:{device}")
    stream = torch.cuda.current_stream(out.device).cuda_stream
    check(L.vrod_synth_rows_device(int(device), int(seed), int(first_row), int(n), int(dim), out.data_ptr(),
                                   C.c_void_p(stream)))
    return out
