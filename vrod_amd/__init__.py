"""vrod_amd -- MI355X (gfx950) brute-force similarity scan + top-k behind vRod's
SEARCHSIMILAR command (sekulas/vRod src/command/types.rs:121-132).

The product is libvrod_hip.so (hand-written HIP, C ABI in include/vrod.h); this package is
the thin harness that loads it.  No CPU or PyTorch fallback exists.
"""
from ._lib import ERR_CAPACITY, ERR_CORRUPT, ERR_IO, LIB_PATH, SYMBOLS, SearchStats, VrodError, load, version  # noqa: F401
from .index import (AGG_BY_LABEL, AGG_BY_TAG, AGG_BY_VALUE, AGG_GROUP_DTYPE, AGG_ORDER_COUNT, MAX_AGG_GROUPS, CENTROID_GROUP_DTYPE, CENTROID_SUM, MAX_CENTROID_GROUPS, DTYPE_BF16, DTYPE_F32, DUP_NARROW_HASH, DUP_WITHIN_LABEL, ID_NONE, MAX_K, METRIC_COSINE, METRIC_IP, METRIC_L2, NEAR_SMALL_POOL,  # noqa: F401
                    ROWFIND_NARROW_HASH, ROWFIND_SMALL_BATCH,
                    PATH_AUTO, PATH_EXACT, PATH_GATHER, PATH_MFMA, PATH_STREAM, SRC_BF16, SRC_F16, SRC_F32, MAX_ORDERED, ORDER_CURSOR_DTYPE, ORDER_DESC, ROWPRED_ALLOWED, ROWPRED_DTYPE, WHERE_DTYPE, Index, merge_topk_device,
                    merge_topk_packed_device, snapshot_info, snapshot_verify, synth_rows_device)

__all__ = ["Index", "VrodError", "merge_topk_device", "merge_topk_packed_device", "synth_rows_device", "snapshot_info", "snapshot_verify", "load", "LIB_PATH", "SYMBOLS"]
