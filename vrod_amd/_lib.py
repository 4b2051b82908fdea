"""ctypes loader for libvrod_hip.so (the C ABI of include/vrod.h).

There is NO Python or CPU fallback: if the shared library is missing or cannot be
loaded this raises, and every entry point fails without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VROD_HIP_LIB: load another build of the same library (A/B timing of two builds in one gpurun call)
LIB_PATH = os.environ.get("VROD_HIP_LIB") or os.path.join(_HERE, "libvrod_hip.so")

# every symbol include/vrod.h declares (tests check the library exports exactly these)
SYMBOLS = [
    "vrod_index_create", "vrod_index_destroy", "vrod_index_reserve", "vrod_index_add",
    "vrod_index_add_synthetic", "vrod_index_count", "vrod_index_set_id_offset",
    "vrod_index_get_rows", "vrod_index_delete", "vrod_index_live_count",
    "vrod_index_set_filter", "vrod_index_filter_count", "vrod_search", "vrod_search_device", "vrod_search_synthetic_device",
    "vrod_search_begin_device", "vrod_search_begin_synthetic_device", "vrod_search_end", "vrod_search_pending",
    "vrod_merge_topk_device", "vrod_merge_topk_packed_device", "vrod_index_set_path", "vrod_index_set_profiling",
    "vrod_index_last_stats", "vrod_index_shard_stats", "vrod_last_error", "vrod_version", "vrod_synth_rows_device",
    "vrod_range_search", "vrod_range_search_device", "vrod_index_update", "vrod_index_compact",
    "vrod_index_set_labels", "vrod_index_get_labels", "vrod_search_labeled", "vrod_search_labeled_device",
    "vrod_search_grouped", "vrod_search_grouped_device",
    "vrod_search_by_ids", "vrod_search_by_ids_device", "vrod_knn_graph",
    "vrod_index_set_tags", "vrod_index_get_tags", "vrod_search_tagged", "vrod_search_tagged_device",
    "vrod_index_set_values", "vrod_index_get_values", "vrod_search_where", "vrod_search_where_device",
    "vrod_search_multivec", "vrod_search_multivec_device", "vrod_index_last_multivec",
    "vrod_search_diverse", "vrod_search_diverse_device",
    "vrod_search_combined", "vrod_search_combined_device",
    "vrod_search_candidates", "vrod_search_candidates_device", "vrod_score_candidates", "vrod_score_candidates_device",
    "vrod_index_save", "vrod_index_load", "vrod_snapshot_info", "vrod_snapshot_verify",
    "vrod_snapshot_checksum", "vrod_snapshot_checksum_device",
    "vrod_index_set_keys", "vrod_index_get_keys", "vrod_index_find_keys", "vrod_index_find_keys_device",
    "vrod_index_ids_to_keys", "vrod_index_ids_to_keys_device", "vrod_index_delete_keys", "vrod_index_upsert",
    "vrod_index_key_stats",
    "vrod_index_add_device", "vrod_index_update_device", "vrod_index_upsert_device", "vrod_index_get_rows_device",
    "vrod_index_count_where", "vrod_index_select_where", "vrod_index_select_where_device", "vrod_index_delete_where",
    "vrod_index_set_filter_where", "vrod_index_set_tags_where",
    "vrod_index_select_ordered", "vrod_index_select_ordered_device",
    "vrod_index_aggregate_where", "vrod_index_centroids_where", "vrod_index_centroids_where_device",
    "vrod_index_find_duplicates", "vrod_index_find_duplicates_device", "vrod_index_delete_duplicates",
    "vrod_index_find_rows", "vrod_index_find_rows_device", "vrod_index_add_unique", "vrod_index_add_unique_device",
    "vrod_index_find_near_duplicates", "vrod_index_find_near_duplicates_device", "vrod_index_delete_near_duplicates",
]

ERR_CAPACITY = 8   # VROD_ERR_CAPACITY: a range search's result does not fit the caller's buffers (out_lims is valid)
ERR_IO = 9         # VROD_ERR_IO: a snapshot's file could not be opened, read, written or renamed
ERR_CORRUPT = 10   # VROD_ERR_CORRUPT: not a snapshot, truncated, sizes that disagree, a checksum mismatch


class VrodError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vrod status {code}: {msg}")
        self.code = code


class SearchStats(C.Structure):
    _fields_ = [
        ("path", C.c_uint32), ("nq", C.c_uint32), ("k", C.c_uint32), ("kprime", C.c_uint32),
        ("scan_launches", C.c_uint32), ("fallback_queries", C.c_uint32),
        ("scan_ms", C.c_float), ("total_ms", C.c_float),
        ("scan_bytes", C.c_double), ("scan_flops", C.c_double),
        ("max_fast_err", C.c_float), ("eps_bound", C.c_float),
        ("split_pass", C.c_uint32), ("band_queries", C.c_uint32), ("sample_ms", C.c_float), ("exchange", C.c_uint32),
        ("overlap_ms", C.c_float),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MultivecStats(C.Structure):
    _fields_ = [
        ("nq", C.c_uint32), ("vectors", C.c_uint32), ("k1", C.c_uint32), ("certified_queries", C.c_uint32),
        ("dense_queries", C.c_uint32), ("candidate_labels", C.c_uint64), ("candidate_rows", C.c_uint64),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SnapshotInfo(C.Structure):
    """struct vrod_snapshot_info: what a snapshot's header says."""
    _fields_ = [
        ("version", C.c_uint32), ("dim", C.c_uint32), ("dtype", C.c_uint32), ("metric", C.c_uint32),
        ("count", C.c_uint64), ("live_count", C.c_uint64), ("id_offset", C.c_uint64), ("file_bytes", C.c_uint64),
        ("has_filter", C.c_uint32), ("has_labels", C.c_uint32), ("has_tags", C.c_uint32), ("has_values", C.c_uint32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KeyStats(C.Structure):
    """vrod_key_stats: the state of a handle's key table."""
    _fields_ = [("keyed_live", C.c_uint64), ("slots", C.c_uint64), ("occupied", C.c_uint64), ("rebuilds", C.c_uint64),
                ("max_probe", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DupStats(C.Structure):
    """vrod_dup_stats: live, classes, duplicates and largest_class are exact; the last three are diagnostics of one call."""
    _fields_ = [("live", C.c_uint64), ("classes", C.c_uint64), ("duplicates", C.c_uint64), ("largest_class", C.c_uint64),
                ("slots", C.c_uint64), ("max_probe", C.c_uint64), ("compare_misses", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RowfindStats(C.Structure):
    """vrod_rowfind_stats: rows, found, repeats and appended are exact; the last four are diagnostics of one call."""
    _fields_ = [("rows", C.c_uint64), ("found", C.c_uint64), ("repeats", C.c_uint64), ("appended", C.c_uint64),
                ("batches", C.c_uint64), ("slots", C.c_uint64), ("max_probe", C.c_uint64), ("compare_misses", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class NearStats(C.Structure):
    """vrod_near_stats: rows, classes, near_duplicates, largest_class and hits are exact; the last three are diagnostics of
    how one call cut its work."""
    _fields_ = [("rows", C.c_uint64), ("classes", C.c_uint64), ("near_duplicates", C.c_uint64), ("largest_class", C.c_uint64),
                ("hits", C.c_uint64), ("batches", C.c_uint64), ("splits", C.c_uint64), ("pool_entries", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.  If torch is
    # going to be used in this process (tests, bench) it must load first so that this library
    # binds to the same runtime; loaded the other way round the second runtime sees no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C vrod_amd/csrc). vrod_amd has no fallback path.")
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.vrod_index_create.argtypes = [C.POINTER(vp), u32, i32, i32, C.POINTER(i32), i32]
    L.vrod_index_destroy.argtypes = [vp]
    L.vrod_index_reserve.argtypes = [vp, u64]
    L.vrod_index_add.argtypes = [vp, vp, u64]
    L.vrod_index_add_synthetic.argtypes = [vp, u64, u64, u64]
    L.vrod_index_count.argtypes = [vp, C.POINTER(u64)]
    L.vrod_index_set_id_offset.argtypes = [vp, u64]
    L.vrod_index_get_rows.argtypes = [vp, u64, u64, vp]
    L.vrod_index_delete.argtypes = [vp, vp, u64]
    L.vrod_index_live_count.argtypes = [vp, C.POINTER(u64)]
    L.vrod_index_update.argtypes = [vp, vp, vp, u64]
    L.vrod_index_compact.argtypes = [vp, vp, u64]
    L.vrod_index_set_filter.argtypes = [vp, vp, u64]
    L.vrod_index_filter_count.argtypes = [vp, C.POINTER(u64)]
    L.vrod_search.argtypes = [vp, vp, u32, u32, vp, vp]
    L.vrod_search_device.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.vrod_search_synthetic_device.argtypes = [vp, u64, u64, u32, u32, vp, vp, vp]
    L.vrod_search_begin_device.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.vrod_search_begin_synthetic_device.argtypes = [vp, u64, u64, u32, u32, vp, vp, vp]
    L.vrod_search_end.argtypes = [vp]
    L.vrod_search_pending.argtypes = [vp, C.POINTER(u32)]
    L.vrod_merge_topk_device.argtypes = [i32, i32, vp, vp, u32, u32, u32, vp, vp, vp]
    L.vrod_merge_topk_packed_device.argtypes = [i32, i32, vp, u32, u32, u32, vp, vp, vp]
    L.vrod_index_set_path.argtypes = [vp, i32]
    L.vrod_index_set_profiling.argtypes = [vp, i32]
    L.vrod_index_last_stats.argtypes = [vp, C.POINTER(SearchStats)]
    L.vrod_index_shard_stats.argtypes = [vp, u32, C.POINTER(i32), C.POINTER(SearchStats)]
    L.vrod_synth_rows_device.argtypes = [i32, u64, u64, u64, u32, vp, vp]
    L.vrod_range_search.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp]
    L.vrod_range_search_device.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp, vp]
    L.vrod_index_set_labels.argtypes = [vp, u64, vp, u64]
    L.vrod_index_get_labels.argtypes = [vp, u64, u64, vp]
    L.vrod_search_labeled.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.vrod_search_labeled_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.vrod_index_set_tags.argtypes = [vp, u64, vp, u64]
    L.vrod_index_get_tags.argtypes = [vp, u64, u64, vp]
    L.vrod_search_tagged.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.vrod_search_tagged_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.vrod_index_set_values.argtypes = [vp, u64, vp, u64]
    L.vrod_index_get_values.argtypes = [vp, u64, u64, vp]
    L.vrod_search_where.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.vrod_search_where_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.vrod_search_grouped.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.vrod_search_grouped_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.vrod_search_by_ids.argtypes = [vp, vp, u32, u32, u32, vp, vp]
    L.vrod_search_by_ids_device.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp]
    L.vrod_knn_graph.argtypes = [vp, u64, u64, u32, vp, vp]
    L.vrod_search_multivec.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    L.vrod_search_multivec_device.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp]
    L.vrod_index_last_multivec.argtypes = [vp, C.POINTER(MultivecStats)]
    L.vrod_search_diverse.argtypes = [vp, vp, u32, u32, u32, C.c_float, vp, vp, vp]
    L.vrod_search_diverse_device.argtypes = [vp, vp, u32, u32, u32, C.c_float, vp, vp, vp, vp]
    L.vrod_search_combined.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp]
    L.vrod_search_combined_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.vrod_search_candidates.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.vrod_search_candidates_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, vp]
    L.vrod_score_candidates.argtypes = [vp, vp, u32, vp, vp, vp]
    L.vrod_score_candidates_device.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    L.vrod_index_save.argtypes = [vp, C.c_char_p]
    L.vrod_index_load.argtypes = [C.POINTER(vp), C.c_char_p, C.POINTER(i32), i32]
    L.vrod_snapshot_info.argtypes = [C.c_char_p, C.POINTER(SnapshotInfo)]
    L.vrod_snapshot_verify.argtypes = [C.c_char_p]
    L.vrod_snapshot_checksum.argtypes = [vp, u64, u64, C.POINTER(u64)]
    L.vrod_snapshot_checksum_device.argtypes = [i32, vp, u64, u64, C.POINTER(u64), vp]
    L.vrod_index_set_keys.argtypes = [vp, u64, vp, u64]
    L.vrod_index_get_keys.argtypes = [vp, u64, u64, vp]
    L.vrod_index_find_keys.argtypes = [vp, vp, u64, vp]
    L.vrod_index_find_keys_device.argtypes = [vp, vp, u64, vp, vp]
    L.vrod_index_ids_to_keys.argtypes = [vp, vp, u64, vp]
    L.vrod_index_ids_to_keys_device.argtypes = [vp, vp, u64, vp, vp]
    L.vrod_index_delete_keys.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.vrod_index_upsert.argtypes = [vp, vp, vp, u64, vp]
    L.vrod_index_key_stats.argtypes = [vp, C.POINTER(KeyStats)]
    L.vrod_index_add_device.argtypes = [vp, vp, i32, u64, u64, vp]
    L.vrod_index_update_device.argtypes = [vp, vp, vp, i32, u64, u64, vp]
    L.vrod_index_upsert_device.argtypes = [vp, vp, vp, i32, u64, u64, vp, vp]
    L.vrod_index_get_rows_device.argtypes = [vp, u64, u64, vp, u64, vp]
    L.vrod_index_count_where.argtypes = [vp, vp, u32, u32, vp]
    L.vrod_index_select_where.argtypes = [vp, vp, u32, u64, C.POINTER(u64), vp]
    L.vrod_index_select_where_device.argtypes = [vp, vp, u32, u64, C.POINTER(u64), vp, vp]
    L.vrod_index_select_ordered.argtypes = [vp, vp, u32, vp, u32, C.POINTER(u64), C.POINTER(u64), vp, vp]
    L.vrod_index_select_ordered_device.argtypes = [vp, vp, u32, vp, u32, C.POINTER(u64), C.POINTER(u64), vp, vp, vp]
    L.vrod_index_aggregate_where.argtypes = [vp, vp, u32, u32, C.c_int64, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
    L.vrod_index_centroids_where.argtypes = [vp, vp, u32, u32, C.c_int64, u32, C.POINTER(u64), C.POINTER(u64), vp, vp, u64]
    L.vrod_index_centroids_where_device.argtypes = [vp, vp, u32, u32, C.c_int64, u32, C.POINTER(u64), C.POINTER(u64), vp, vp, u64, vp]
    L.vrod_index_delete_where.argtypes = [vp, vp, u32, C.POINTER(u64)]
    L.vrod_index_set_filter_where.argtypes = [vp, vp, u32]
    L.vrod_index_set_tags_where.argtypes = [vp, vp, u32, u64, u64, C.POINTER(u64)]
    L.vrod_index_find_duplicates.argtypes = [vp, u32, vp, u64, C.POINTER(DupStats)]
    L.vrod_index_find_duplicates_device.argtypes = [vp, u32, vp, u64, C.POINTER(DupStats), vp]
    L.vrod_index_delete_duplicates.argtypes = [vp, u32, C.POINTER(u64)]
    L.vrod_index_find_rows.argtypes = [vp, vp, u64, u32, vp, C.POINTER(RowfindStats)]
    L.vrod_index_find_rows_device.argtypes = [vp, vp, i32, u64, u64, u32, vp, C.POINTER(RowfindStats), vp]
    L.vrod_index_add_unique.argtypes = [vp, vp, u64, u32, vp, C.POINTER(RowfindStats)]
    L.vrod_index_add_unique_device.argtypes = [vp, vp, i32, u64, u64, u32, vp, C.POINTER(RowfindStats), vp]
    L.vrod_index_find_near_duplicates.argtypes = [vp, C.c_float, u32, vp, u64, C.POINTER(NearStats)]
    L.vrod_index_find_near_duplicates_device.argtypes = [vp, C.c_float, u32, vp, u64, C.POINTER(NearStats), vp]
    L.vrod_index_delete_near_duplicates.argtypes = [vp, C.c_float, u32, C.POINTER(u64)]
    for name in SYMBOLS:
        getattr(L, name).restype = i32
    L.vrod_last_error.restype = C.c_char_p
    L.vrod_last_error.argtypes = []
    L.vrod_version.restype = C.c_char_p
    L.vrod_version.argtypes = []
    _lib = L
    return L


def version() -> str:
    """vrod_version(): library version + the hipcc that built the device code."""
    return load().vrod_version().decode()


def check(rc: int) -> None:
    if rc != 0:
        raise VrodError(rc, load().vrod_last_error().decode("utf-8", "replace"))
