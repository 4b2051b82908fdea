//! FFI declarations + a safe wrapper for `libvrod_hip.so` (C ABI: `include/vrod.h`).
//!
//! This is the binding a vRod maintainer would add so that `SearchSimilarCommand::execute`
//! (reference `src/command/types.rs:121-132`, an empty stub) and `BulkInsertCommand::execute`
//! (`types.rs:69-80`) can call the MI355X scan.  Source only: there is no Rust toolchain in the
//! image this repository is built in, so this crate has never been compiled here.
#![allow(non_camel_case_types)]
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct vrod_index {
    _private: [u8; 0],
}

pub const VROD_DTYPE_F32: c_int = 0;
pub const VROD_DTYPE_BF16: c_int = 1;
pub const VROD_METRIC_COSINE: c_int = 0;
pub const VROD_METRIC_L2: c_int = 1;
pub const VROD_METRIC_IP: c_int = 2;
pub const VROD_ID_NONE: u64 = u64::MAX;
pub const VROD_MAX_K: u32 = 3584;
pub const VROD_PATH_AUTO: c_int = 0;
pub const VROD_PATH_STREAM: c_int = 1;
pub const VROD_PATH_MFMA: c_int = 2;
pub const VROD_PATH_EXACT: c_int = 3;
/// Filtered searches: canonical scores of the eligible rows only.
pub const VROD_PATH_GATHER: c_int = 4;
/// `vrod_range_search`: the result does not fit the caller's buffers (`out_lims` is valid).
pub const VROD_ERR_CAPACITY: c_int = 8;
/// Snapshots: open / read / write / rename / fsync failed.
pub const VROD_ERR_IO: c_int = 9;
/// Snapshots: not a snapshot, a truncated file, sizes that disagree, a checksum mismatch.
pub const VROD_ERR_CORRUPT: c_int = 10;

/// What a snapshot's header says (`vrod_snapshot_info`; a struct tag in C, the function has the same name).
#[repr(C)]
#[derive(Debug, Default, Clone, Copy, PartialEq, Eq)]
pub struct vrod_snapshot_info {
    pub version: u32,
    pub dim: u32,
    pub dtype: u32,
    pub metric: u32,
    pub count: u64,
    pub live_count: u64,
    pub id_offset: u64,
    pub file_bytes: u64,
    pub has_filter: u32,
    pub has_labels: u32,
    pub has_tags: u32,
    pub has_values: u32,
}

#[repr(C)]
#[derive(Debug, Default, Clone, Copy)]
pub struct vrod_search_stats {
    pub path: u32,
    pub nq: u32,
    pub k: u32,
    pub kprime: u32,
    pub scan_launches: u32,
    pub fallback_queries: u32,
    pub scan_ms: f32,
    pub total_ms: f32,
    pub scan_bytes: f64,
    pub scan_flops: f64,
    pub max_fast_err: f32,
    pub eps_bound: f32,
    /// 1: the batched fast pass of an F32 handle ran on its bf16 [hi | lo] planes
    pub split_pass: u32,
    pub band_queries: u32,
    pub sample_ms: f32,
    pub exchange: u32,
    pub overlap_ms: f32,
}

/// One query's predicate over the 64 tag bits of a row (`vrod_search_tagged`): a row with tags `t` matches iff
/// `(any == 0 || t & any != 0) && t & all == all && t & none == 0`.
#[repr(C)]
#[derive(Debug, Default, Clone, Copy, PartialEq, Eq)]
pub struct vrod_tag_pred {
    pub any: u64,
    pub all: u64,
    pub none: u64,
}

/// One query's predicate of `vrod_search_where`: the tag clauses of `vrod_tag_pred` and `lo <= v && v <= hi` on the row's
/// signed 64-bit value `v`, both ends inclusive.
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct vrod_where {
    pub any: u64,
    pub all: u64,
    pub none: u64,
    pub lo: i64,
    pub hi: i64,
}

/// The predicate of the row-predicate operations (`vrod_index_count_where` ... `vrod_index_set_tags_where`): the clauses of
/// `vrod_where` and, when `has_label` is 1, `label == l` on the row's label `l`.  48 bytes, no padding.
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct vrod_row_pred {
    pub any: u64,
    pub all: u64,
    pub none: u64,
    pub lo: i64,
    pub hi: i64,
    pub label: u32,
    pub has_label: u32,
}
/// `flags` of the row-predicate operations: only the rows the handle's filter allows are in scope.
pub const VROD_ROWPRED_ALLOWED: u32 = 1;

/// `flags` bit of `vrod_index_select_ordered`: value descending (ids still ascending among equal values).  Shares the
/// word with `VROD_ROWPRED_ALLOWED`.
pub const VROD_ORDER_DESC: u32 = 2;
/// Rows one `vrod_index_select_ordered` call returns; longer listings page with the cursor.
pub const VROD_MAX_ORDERED: u32 = 65536;
/// The keyset cursor of `vrod_index_select_ordered`: the last (value, id) of the page before.  16 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vrod_order_cursor {
    pub value: i64,
    pub id: u64,
}

/// `by` of `vrod_index_aggregate_where`: the key of a group is the row's label (0 .. 2^32-1).
pub const VROD_AGG_BY_LABEL: u32 = 0;
/// ... floor(value / width): floor division on signed values, width >= 1.
pub const VROD_AGG_BY_VALUE: u32 = 1;
/// ... a bit index 0..63: a row counts in the group of EVERY tag bit it has set.
pub const VROD_AGG_BY_TAG: u32 = 2;
/// `flags` bit of `vrod_index_aggregate_where`: groups by count descending, then key ascending.  Shares the word with
/// `VROD_ROWPRED_ALLOWED`; 2 stays `VROD_ORDER_DESC`'s and is refused there.
pub const VROD_AGG_ORDER_COUNT: u32 = 4;
/// Distinct groups one `vrod_index_aggregate_where` call holds; more is `VROD_ERR_CAPACITY`.
pub const VROD_MAX_AGG_GROUPS: u32 = 1048576;
/// One group of `vrod_index_aggregate_where`: its key, its rows, the min, max and wrapping sum of their values and the
/// smallest id among them (id_offset applied).  48 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vrod_agg_group {
    pub key: i64,
    pub count: u64,
    pub min_value: i64,
    pub max_value: i64,
    pub sum_value: i64,
    pub first_id: u64,
}

/// `flags` bit of `vrod_index_centroids_where`: each group's sum, not its mean.  Shares the word with `VROD_ROWPRED_ALLOWED`.
pub const VROD_CENTROID_SUM: u32 = 8;
/// Groups one `vrod_index_centroids_where` call holds; more than the call's capacity is `VROD_ERR_CAPACITY`.
pub const VROD_MAX_CENTROID_GROUPS: u32 = 65536;
/// One group of `vrod_index_centroids_where`: its key, its rows and the smallest id among them (id_offset applied), as
/// `vrod_index_aggregate_where` reports them.  24 bytes, no padding.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vrod_centroid_group {
    pub key: i64,
    pub count: u64,
    pub first_id: u64,
}

/// `flags` of the duplicate-row calls: the class key is (label, row bits), so equal rows of two documents stay apart.
pub const VROD_DUP_WITHIN_LABEL: u32 = 1;
/// A diagnostic for tests: the row hash is cut to 8 bits; results are identical with and without it.
pub const VROD_DUP_NARROW_HASH: u32 = 0x8000_0000;
/// What `vrod_index_find_duplicates` reports: the first four fields are exact and reproducible, the last three are
/// diagnostics of one call's hash table.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct vrod_dup_stats {
    pub live: u64,
    pub classes: u64,
    pub duplicates: u64,
    pub largest_class: u64,
    pub slots: u64,
    pub max_probe: u64,
    pub compare_misses: u64,
}

/// `flags` of the row-lookup calls.  Diagnostics for tests: the row hash is cut to 8 bits (as `VROD_DUP_NARROW_HASH`); the
/// call's lookup batches hold 96 rows.  Results are identical with and without them.
pub const VROD_ROWFIND_NARROW_HASH: u32 = 0x8000_0000;
pub const VROD_ROWFIND_SMALL_BATCH: u32 = 0x4000_0000;
/// What `vrod_index_find_rows` and `vrod_index_add_unique` report: the first four fields are exact and reproducible, the
/// last four are diagnostics of how one call cut its work and of its hash tables.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct vrod_rowfind_stats {
    pub rows: u64,
    pub found: u64,
    pub repeats: u64,
    pub appended: u64,
    pub batches: u64,
    pub slots: u64,
    pub max_probe: u64,
    pub compare_misses: u64,
}

/// `flags` of the near-duplicate calls.  A diagnostic for tests: the hit pool of the call holds exactly as many entries as
/// there are eligible rows, so batches split on a small corpus; results are identical with and without it.
pub const VROD_NEAR_SMALL_POOL: u32 = 0x8000_0000;
/// What `vrod_index_find_near_duplicates` reports: the first five fields are exact and reproducible, the last three are
/// diagnostics of how one call cut its work.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq, Eq)]
pub struct vrod_near_stats {
    pub rows: u64,
    pub classes: u64,
    pub near_duplicates: u64,
    pub largest_class: u64,
    pub hits: u64,
    pub batches: u64,
    pub splits: u64,
    pub pool_entries: u64,
}

/// The largest `pool` of `vrod_search_diverse`.
pub const VROD_MAX_DIVERSE_POOL: u32 = 1024;

/// `vrod_search_combined`: the most stored-row terms, and the most excluded ids (terms included under the flag), of one query.
pub const VROD_MAX_COMBINE_TERMS: u32 = 256;
pub const VROD_MAX_EXCLUDE: u32 = 1024;
/// `flags` of `vrod_search_combined`: a query's term ids are excluded from its result.
pub const VROD_COMBINED_EXCLUDE_TERMS: u32 = 1;

/// The most list entries one query of `vrod_search_candidates` / `vrod_score_candidates` may hold.
pub const VROD_MAX_CANDIDATES: u32 = 16384;

/// The most vectors one query of `vrod_search_multivec` may hold.
pub const VROD_MAX_QUERY_VECTORS: u32 = 256;

/// What the last `vrod_search_multivec` call did (`vrod_index_last_multivec`): `certified_queries` were answered by the
/// candidate route, `dense_queries` by the dense route; `k1` is 0 when no first-stage search ran.
#[repr(C)]
#[derive(Debug, Default, Clone, Copy, PartialEq, Eq)]
pub struct vrod_multivec_stats {
    pub nq: u32,
    pub vectors: u32,
    pub k1: u32,
    pub certified_queries: u32,
    pub dense_queries: u32,
    pub candidate_labels: u64,
    pub candidate_rows: u64,
}

/// `vrod_key_stats`: the state of a handle's key table.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct vrod_key_stats {
    pub keyed_live: u64,
    pub slots: u64,
    pub occupied: u64,
    pub rebuilds: u64,
    pub max_probe: u64,
}

extern "C" {
    pub fn vrod_index_create(out: *mut *mut vrod_index, dim: u32, dtype: c_int, metric: c_int,
                             device_ids: *const c_int, n_devices: c_int) -> c_int;
    pub fn vrod_index_destroy(idx: *mut vrod_index) -> c_int;
    pub fn vrod_index_reserve(idx: *mut vrod_index, n_rows: u64) -> c_int;
    pub fn vrod_index_add(idx: *mut vrod_index, rows: *const f32, n: u64) -> c_int;
    pub fn vrod_index_add_synthetic(idx: *mut vrod_index, seed: u64, first_row: u64, n: u64) -> c_int;
    pub fn vrod_index_count(idx: *const vrod_index, out_count: *mut u64) -> c_int;
    pub fn vrod_index_set_id_offset(idx: *mut vrod_index, offset: u64) -> c_int;
    pub fn vrod_index_get_rows(idx: *mut vrod_index, first: u64, n: u64, out_rows: *mut f32) -> c_int;
    pub fn vrod_index_delete(idx: *mut vrod_index, ids: *const u64, n: u64) -> c_int;
    pub fn vrod_index_live_count(idx: *const vrod_index, out: *mut u64) -> c_int;
    pub fn vrod_index_update(idx: *mut vrod_index, ids: *const u64, rows: *const f32, n: u64) -> c_int;
    pub fn vrod_index_compact(idx: *mut vrod_index, out_new_ids: *mut u64, map_len: u64) -> c_int;
    pub fn vrod_index_set_filter(idx: *mut vrod_index, allow_words: *const u32, n_rows: u64) -> c_int;
    pub fn vrod_index_filter_count(idx: *const vrod_index, out: *mut u64) -> c_int;
    pub fn vrod_search(idx: *mut vrod_index, queries: *const f32, nq: u32, k: u32,
                       out_ids: *mut u64, out_scores: *mut f32) -> c_int;
    pub fn vrod_search_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32,
                              d_out_ids: *mut u64, d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    pub fn vrod_search_synthetic_device(idx: *mut vrod_index, seed: u64, first_row: u64, nq: u32, k: u32,
                                        d_out_ids: *mut u64, d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    pub fn vrod_search_begin_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32,
                                    d_out_ids: *mut u64, d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    pub fn vrod_search_begin_synthetic_device(idx: *mut vrod_index, seed: u64, first_row: u64, nq: u32, k: u32,
                                              d_out_ids: *mut u64, d_out_scores: *mut f32,
                                              stream: *mut c_void) -> c_int;
    pub fn vrod_search_end(idx: *mut vrod_index) -> c_int;
    pub fn vrod_search_pending(idx: *const vrod_index, out_pending: *mut u32) -> c_int;
    pub fn vrod_merge_topk_device(device: c_int, metric: c_int, d_ids: *const u64, d_scores: *const f32,
                                  n_lists: u32, nq: u32, k: u32, d_out_ids: *mut u64,
                                  d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    pub fn vrod_merge_topk_packed_device(device: c_int, metric: c_int, d_packed: *const c_void, n_lists: u32,
                                         nq: u32, k: u32, d_out_ids: *mut u64, d_out_scores: *mut f32,
                                         stream: *mut c_void) -> c_int;
    pub fn vrod_index_set_path(idx: *mut vrod_index, path: c_int) -> c_int;
    pub fn vrod_index_set_profiling(idx: *mut vrod_index, on: c_int) -> c_int;
    pub fn vrod_index_last_stats(idx: *const vrod_index, out: *mut vrod_search_stats) -> c_int;
    pub fn vrod_index_shard_stats(idx: *const vrod_index, shard: u32, out_device: *mut c_int,
                                  out: *mut vrod_search_stats) -> c_int;
    pub fn vrod_last_error() -> *const c_char;
    pub fn vrod_version() -> *const c_char;
    pub fn vrod_synth_rows_device(device: c_int, seed: u64, first_row: u64, n: u64, dim: u32,
                                  d_out: *mut f32, stream: *mut c_void) -> c_int;
    pub fn vrod_range_search(idx: *mut vrod_index, queries: *const f32, nq: u32, thresholds: *const f32,
                             capacity: u64, out_lims: *mut u64, out_ids: *mut u64, out_scores: *mut f32) -> c_int;
    pub fn vrod_range_search_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, d_thresholds: *const f32,
                                    capacity: u64, d_out_lims: *mut u64, d_out_ids: *mut u64,
                                    d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    pub fn vrod_index_set_labels(idx: *mut vrod_index, first_id: u64, labels: *const u32, n: u64) -> c_int;
    pub fn vrod_index_get_labels(idx: *mut vrod_index, first_id: u64, n: u64, out_labels: *mut u32) -> c_int;
    pub fn vrod_search_labeled(idx: *mut vrod_index, queries: *const f32, nq: u32, k: u32, query_labels: *const u32,
                               out_ids: *mut u64, out_scores: *mut f32) -> c_int;
    pub fn vrod_search_labeled_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32,
                                      d_query_labels: *const u32, d_out_ids: *mut u64, d_out_scores: *mut f32,
                                      stream: *mut c_void) -> c_int;
    pub fn vrod_search_grouped(idx: *mut vrod_index, queries: *const f32, nq: u32, k: u32, out_ids: *mut u64,
                               out_scores: *mut f32, out_labels: *mut u32) -> c_int;
    pub fn vrod_search_grouped_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32, d_out_ids: *mut u64,
                                      d_out_scores: *mut f32, d_out_labels: *mut u32, stream: *mut c_void) -> c_int;
    pub fn vrod_index_set_tags(idx: *mut vrod_index, first_id: u64, tags: *const u64, n: u64) -> c_int;
    pub fn vrod_index_get_tags(idx: *mut vrod_index, first_id: u64, n: u64, out_tags: *mut u64) -> c_int;
    pub fn vrod_search_tagged(idx: *mut vrod_index, queries: *const f32, nq: u32, k: u32, preds: *const vrod_tag_pred,
                              out_ids: *mut u64, out_scores: *mut f32) -> c_int;
    pub fn vrod_search_tagged_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32,
                                     d_preds: *const vrod_tag_pred, d_out_ids: *mut u64, d_out_scores: *mut f32,
                                     stream: *mut c_void) -> c_int;
    pub fn vrod_index_set_values(idx: *mut vrod_index, first_id: u64, values: *const i64, n: u64) -> c_int;
    pub fn vrod_index_get_values(idx: *mut vrod_index, first_id: u64, n: u64, out_values: *mut i64) -> c_int;
    pub fn vrod_search_where(idx: *mut vrod_index, queries: *const f32, nq: u32, k: u32, preds: *const vrod_where,
                             out_ids: *mut u64, out_scores: *mut f32) -> c_int;
    pub fn vrod_search_where_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32,
                                    d_preds: *const vrod_where, d_out_ids: *mut u64, d_out_scores: *mut f32,
                                    stream: *mut c_void) -> c_int;
    /// `flags`: 0, or 1 (`VROD_BYID_EXCLUDE_SELF`): the row itself is no candidate of its own query.
    pub fn vrod_search_by_ids(idx: *mut vrod_index, ids: *const u64, nq: u32, k: u32, flags: u32, out_ids: *mut u64,
                              out_scores: *mut f32) -> c_int;
    pub fn vrod_search_by_ids_device(idx: *mut vrod_index, d_ids: *const u64, nq: u32, k: u32, flags: u32,
                                     d_out_ids: *mut u64, d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    pub fn vrod_knn_graph(idx: *mut vrod_index, first_id: u64, n: u64, k: u32, out_ids: *mut u64,
                          out_scores: *mut f32) -> c_int;
    /// Query q owns vectors `query_lims[q] .. query_lims[q + 1]`; `out_found` may be null.
    pub fn vrod_search_multivec(idx: *mut vrod_index, vectors: *const f32, query_lims: *const u32, nq: u32, k: u32,
                                out_labels: *mut u32, out_scores: *mut f32, out_found: *mut u32) -> c_int;
    pub fn vrod_search_multivec_device(idx: *mut vrod_index, d_vectors: *const f32, d_query_lims: *const u32, nq: u32,
                                       k: u32, d_out_labels: *mut u32, d_out_scores: *mut f32, d_out_found: *mut u32,
                                       stream: *mut c_void) -> c_int;
    pub fn vrod_index_last_multivec(idx: *const vrod_index, out: *mut vrod_multivec_stats) -> c_int;
    /// Exact greedy MMR over the certified top `pool`; rows come back in selection order; `out_mmr` may be null.
    pub fn vrod_search_diverse(idx: *mut vrod_index, queries: *const f32, nq: u32, k: u32, pool: u32, lambda: f32,
                               out_ids: *mut u64, out_scores: *mut f32, out_mmr: *mut f32) -> c_int;
    pub fn vrod_search_diverse_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32, pool: u32, lambda: f32,
                                      d_out_ids: *mut u64, d_out_scores: *mut f32, d_out_mmr: *mut f32,
                                      stream: *mut c_void) -> c_int;
    /// Query q = its prepared vector (if `vectors` is not null) and the stored rows `term_ids[term_lims[q] .. term_lims[q + 1]]`,
    /// weighted and added in order; its result leaves out `exclude_ids[exclude_lims[q] .. exclude_lims[q + 1]]` (both may be
    /// null) and, with `VROD_COMBINED_EXCLUDE_TERMS`, the terms.
    pub fn vrod_search_combined(idx: *mut vrod_index, vectors: *const f32, vector_weights: *const f32, term_lims: *const u32,
                                term_ids: *const u64, term_weights: *const f32, exclude_lims: *const u32,
                                exclude_ids: *const u64, nq: u32, k: u32, flags: u32, out_ids: *mut u64,
                                out_scores: *mut f32) -> c_int;
    pub fn vrod_search_combined_device(idx: *mut vrod_index, d_vectors: *const f32, d_vector_weights: *const f32,
                                       d_term_lims: *const u32, d_term_ids: *const u64, d_term_weights: *const f32,
                                       d_exclude_lims: *const u32, d_exclude_ids: *const u64, nq: u32, k: u32, flags: u32,
                                       d_out_ids: *mut u64, d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    /// Query q sees only the rows `cand_ids[cand_lims[q] .. cand_lims[q + 1]]` name (any order; repeats, deleted, disallowed
    /// and stale ids are ignored): its exact top k among them.
    pub fn vrod_search_candidates(idx: *mut vrod_index, queries: *const f32, nq: u32, k: u32, cand_lims: *const u32,
                                  cand_ids: *const u64, out_ids: *mut u64, out_scores: *mut f32) -> c_int;
    pub fn vrod_search_candidates_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, k: u32,
                                         d_cand_lims: *const u32, d_cand_ids: *const u64, d_out_ids: *mut u64,
                                         d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    /// `out_scores[t]` = the canonical score of query q against row `cand_ids[t]`, NaN where the id is ignored.
    pub fn vrod_score_candidates(idx: *mut vrod_index, queries: *const f32, nq: u32, cand_lims: *const u32,
                                 cand_ids: *const u64, out_scores: *mut f32) -> c_int;
    pub fn vrod_score_candidates_device(idx: *mut vrod_index, d_queries: *const f32, nq: u32, d_cand_lims: *const u32,
                                        d_cand_ids: *const u64, d_out_scores: *mut f32, stream: *mut c_void) -> c_int;
    /// Snapshots: the whole observable state of a single-device handle in one file, and back (`Database::load`).
    pub fn vrod_index_save(idx: *mut vrod_index, path: *const c_char) -> c_int;
    pub fn vrod_index_load(out: *mut *mut vrod_index, path: *const c_char, device_ids: *const c_int, n_devices: c_int) -> c_int;
    pub fn vrod_snapshot_info(path: *const c_char, out: *mut vrod_snapshot_info) -> c_int;
    pub fn vrod_snapshot_verify(path: *const c_char) -> c_int;
    pub fn vrod_snapshot_checksum(bytes: *const c_void, n_bytes: u64, first_word: u64, out: *mut u64) -> c_int;
    pub fn vrod_snapshot_checksum_device(device: c_int, d_bytes: *const c_void, n_bytes: u64, first_word: u64, out: *mut u64,
                                         stream: *mut c_void) -> c_int;
    /// Row keys: caller-chosen 64-bit names that survive `vrod_index_compact`, unique among the live rows.
    pub fn vrod_index_set_keys(idx: *mut vrod_index, first_id: u64, keys: *const u64, n: u64) -> c_int;
    pub fn vrod_index_get_keys(idx: *mut vrod_index, first_id: u64, n: u64, out_keys: *mut u64) -> c_int;
    pub fn vrod_index_find_keys(idx: *mut vrod_index, keys: *const u64, n: u64, out_ids: *mut u64) -> c_int;
    pub fn vrod_index_find_keys_device(idx: *mut vrod_index, d_keys: *const u64, n: u64, d_out_ids: *mut u64, stream: *mut c_void) -> c_int;
    pub fn vrod_index_ids_to_keys(idx: *mut vrod_index, ids: *const u64, n: u64, out_keys: *mut u64) -> c_int;
    pub fn vrod_index_ids_to_keys_device(idx: *mut vrod_index, d_ids: *const u64, n: u64, d_out_keys: *mut u64, stream: *mut c_void) -> c_int;
    pub fn vrod_index_delete_keys(idx: *mut vrod_index, keys: *const u64, n: u64, out_deleted: *mut u64) -> c_int;
    pub fn vrod_index_upsert(idx: *mut vrod_index, keys: *const u64, rows: *const f32, n: u64, out_ids: *mut u64) -> c_int;
    pub fn vrod_index_key_stats(idx: *const vrod_index, out: *mut vrod_key_stats) -> c_int;
    /// Device-resident ingest: `src_dtype` is 0 (f32), 1 (bf16) or 2 (f16); `row_stride` is in elements, `>= dim`.
    pub fn vrod_index_add_device(idx: *mut vrod_index, d_rows: *const c_void, src_dtype: c_int, row_stride: u64, n: u64, stream: *mut c_void) -> c_int;
    pub fn vrod_index_update_device(idx: *mut vrod_index, d_ids: *const u64, d_rows: *const c_void, src_dtype: c_int, row_stride: u64, n: u64, stream: *mut c_void) -> c_int;
    pub fn vrod_index_upsert_device(idx: *mut vrod_index, d_keys: *const u64, d_rows: *const c_void, src_dtype: c_int, row_stride: u64, n: u64, d_out_ids: *mut u64, stream: *mut c_void) -> c_int;
    pub fn vrod_index_get_rows_device(idx: *mut vrod_index, first: u64, n: u64, d_out_rows: *mut f32, out_row_stride: u64, stream: *mut c_void) -> c_int;
    /// Row predicates: `flags` is 0 or `VROD_ROWPRED_ALLOWED`; the columns are read on the device.
    pub fn vrod_index_count_where(idx: *mut vrod_index, preds: *const vrod_row_pred, n_preds: u32, flags: u32, out_counts: *mut u64) -> c_int;
    pub fn vrod_index_select_where(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, capacity: u64, out_count: *mut u64, out_ids: *mut u64) -> c_int;
    pub fn vrod_index_select_where_device(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, capacity: u64, out_count: *mut u64, d_out_ids: *mut u64, stream: *mut c_void) -> c_int;
    pub fn vrod_index_delete_where(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, out_deleted: *mut u64) -> c_int;
    pub fn vrod_index_set_filter_where(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32) -> c_int;
    pub fn vrod_index_set_tags_where(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, set_bits: u64, clear_bits: u64, out_changed: *mut u64) -> c_int;
    /// Ordered selection: the first `limit` rows `select_where` lists by (value, id), `VROD_ORDER_DESC` in `flags` for
    /// value descending, strictly after `after` (null: from the beginning).  `*out_count` = min(limit, `*out_total`);
    /// `out_total` and `out_values` may be null.  The `_device` form writes the two arrays to device memory.
    pub fn vrod_index_select_ordered(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, after: *const vrod_order_cursor, limit: u32, out_count: *mut u64, out_total: *mut u64, out_ids: *mut u64, out_values: *mut i64) -> c_int;
    pub fn vrod_index_select_ordered_device(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, after: *const vrod_order_cursor, limit: u32, out_count: *mut u64, out_total: *mut u64, d_out_ids: *mut u64, d_out_values: *mut i64, stream: *mut c_void) -> c_int;
    /// Row aggregation, the GROUP BY of the row predicates: the rows `select_where` lists grouped by label, value bucket
    /// or tag bit (`by`), per group the count, min / max / wrapping sum of the values and the smallest id; `out` holds the
    /// first `min(limit, groups)` groups by key, or with `VROD_AGG_ORDER_COUNT` by count descending.
    pub fn vrod_index_aggregate_where(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, by: u32, width: i64, limit: u32, out_count: *mut u64, out_groups: *mut u64, out_rows: *mut u64, out: *mut vrod_agg_group) -> c_int;
    /// Group centroids: the exact, order-free mean (`VROD_CENTROID_SUM`: sum) of the rows of every group of the rows
    /// `select_where` lists, the groups by label or value bucket in ascending key order; group g's `dim` floats start at
    /// `out_vectors + g * out_row_stride`.  The `_device` form leaves the vectors in device memory.
    pub fn vrod_index_centroids_where(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, by: u32, width: i64, capacity: u32, out_count: *mut u64, out_rows: *mut u64, out_groups: *mut vrod_centroid_group, out_vectors: *mut f32, out_row_stride: u64) -> c_int;
    pub fn vrod_index_centroids_where_device(idx: *mut vrod_index, pred: *const vrod_row_pred, flags: u32, by: u32, width: i64, capacity: u32, out_count: *mut u64, out_rows: *mut u64, out_groups: *mut vrod_centroid_group, d_out_vectors: *mut f32, out_row_stride: u64, stream: *mut c_void) -> c_int;
    /// Duplicate rows: `out_first[i]` = the smallest id among the live rows whose stored bits equal row i's (`map_len` =
    /// `vrod_index_count`, or null and 0 for the stats alone); `delete_duplicates` keeps that smallest id of every class.
    pub fn vrod_index_find_duplicates(idx: *mut vrod_index, flags: u32, out_first: *mut u64, map_len: u64, out_stats: *mut vrod_dup_stats) -> c_int;
    pub fn vrod_index_find_duplicates_device(idx: *mut vrod_index, flags: u32, d_out_first: *mut u64, map_len: u64, out_stats: *mut vrod_dup_stats, stream: *mut c_void) -> c_int;
    pub fn vrod_index_delete_duplicates(idx: *mut vrod_index, flags: u32, out_deleted: *mut u64) -> c_int;
    /// Row lookup: `out_ids[i]` (may be null) = the smallest id among the live rows whose stored bits equal input i as
    /// `vrod_index_add` would store it, `VROD_ID_NONE` if there is none.  `add_unique` appends the inputs that have no stored
    /// copy and repeat no earlier input of the call, and names every input's row.
    pub fn vrod_index_find_rows(idx: *mut vrod_index, rows: *const f32, n: u64, flags: u32, out_ids: *mut u64, out_stats: *mut vrod_rowfind_stats) -> c_int;
    pub fn vrod_index_find_rows_device(idx: *mut vrod_index, d_rows: *const c_void, src_dtype: c_int, row_stride: u64, n: u64, flags: u32, d_out_ids: *mut u64, out_stats: *mut vrod_rowfind_stats, stream: *mut c_void) -> c_int;
    pub fn vrod_index_add_unique(idx: *mut vrod_index, rows: *const f32, n: u64, flags: u32, out_ids: *mut u64, out_stats: *mut vrod_rowfind_stats) -> c_int;
    pub fn vrod_index_add_unique_device(idx: *mut vrod_index, d_rows: *const c_void, src_dtype: c_int, row_stride: u64, n: u64, flags: u32, d_out_ids: *mut u64, out_stats: *mut vrod_rowfind_stats, stream: *mut c_void) -> c_int;
    /// Near-duplicate rows: `out_first[i]` = the smallest id of row i's class, the connected component -- among the eligible
    /// rows: live, allowed by the filter -- of the graph that joins two rows when one's stored form scores the other at
    /// least as well as `threshold` (single linkage: a~b and b~c put a and c together).  `map_len` as for
    /// `vrod_index_find_duplicates`; `delete_near_duplicates` keeps the smallest id of every class.
    pub fn vrod_index_find_near_duplicates(idx: *mut vrod_index, threshold: f32, flags: u32, out_first: *mut u64, map_len: u64, out_stats: *mut vrod_near_stats) -> c_int;
    pub fn vrod_index_find_near_duplicates_device(idx: *mut vrod_index, threshold: f32, flags: u32, d_out_first: *mut u64, map_len: u64, out_stats: *mut vrod_near_stats, stream: *mut c_void) -> c_int;
    pub fn vrod_index_delete_near_duplicates(idx: *mut vrod_index, threshold: f32, flags: u32, out_deleted: *mut u64) -> c_int;
}

/// Joins the reference's `thiserror` enums (`src/main.rs:36-40`, `src/command/builder.rs:10-15`).
#[derive(Debug, thiserror::Error)]
pub enum ScanError {
    #[error("vrod_hip status {0}: {1}")]
    Device(i32, String),
    #[error("vector has {got} values, collection dimension is {want}")]
    Dim { got: usize, want: usize },
}

fn check(rc: c_int) -> Result<(), ScanError> {
    if rc == 0 {
        return Ok(());
    }
    let msg = unsafe { CStr::from_ptr(vrod_last_error()) }.to_string_lossy().into_owned();
    Err(ScanError::Device(rc, msg))
}

#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Metric { Cosine, L2, InnerProduct }
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Dtype { F32, Bf16 }

/// One collection's vectors in HBM.  `!Send + !Sync`, like the reference's `Rc<RefCell<Database>>`
/// (`src/command/types.rs:10`): calls on one handle are serialised by construction.
pub struct Collection {
    idx: *mut vrod_index,
    dim: usize,
}

impl Collection {
    pub fn new(dim: usize, dtype: Dtype, metric: Metric) -> Result<Self, ScanError> {
        let mut idx = std::ptr::null_mut();
        let dt = if dtype == Dtype::Bf16 { VROD_DTYPE_BF16 } else { VROD_DTYPE_F32 };
        let me = match metric {
            Metric::Cosine => VROD_METRIC_COSINE,
            Metric::L2 => VROD_METRIC_L2,
            Metric::InnerProduct => VROD_METRIC_IP,
        };
        check(unsafe { vrod_index_create(&mut idx, dim as u32, dt, me, std::ptr::null(), 0) })?;
        Ok(Self { idx, dim })
    }

    /// `embeddings` is the reference's own type (`src/utils/embeddings.rs:29`).
    pub fn add(&mut self, embeddings: &[Vec<f32>]) -> Result<(), ScanError> {
        let mut flat = Vec::with_capacity(embeddings.len() * self.dim);
        for e in embeddings {
            if e.len() != self.dim {
                return Err(ScanError::Dim { got: e.len(), want: self.dim });
            }
            flat.extend_from_slice(e);
        }
        check(unsafe { vrod_index_add(self.idx, flat.as_ptr(), embeddings.len() as u64) })
    }

    pub fn len(&self) -> u64 {
        let mut n = 0u64;
        unsafe { vrod_index_count(self.idx, &mut n) };
        n
    }

    /// Deletes rows by the ids `search` reports (`DeleteCommand::execute`).  An id that is not a row fails the whole
    /// call and deletes nothing; deleting a row twice is fine.  Ids are never reused until `compact` renumbers them:
    /// `len()` still counts them.
    pub fn delete(&mut self, ids: &[u64]) -> Result<(), ScanError> {
        check(unsafe { vrod_index_delete(self.idx, ids.as_ptr(), ids.len() as u64) })
    }

    /// Gives row `ids[i]` the vector `embeddings[i]` in place (`UpdateCommand::execute`): the row keeps its id and
    /// the vector is prepared as `add` prepares it.  An id that is not a current row (a deleted one included) or a
    /// NaN / Inf fails the whole call and changes nothing; an id named twice takes the last vector.
    pub fn update(&mut self, ids: &[u64], embeddings: &[Vec<f32>]) -> Result<(), ScanError> {
        if embeddings.len() != ids.len() {
            return Err(ScanError::Dim { got: embeddings.len(), want: ids.len() });
        }
        let mut flat = Vec::with_capacity(embeddings.len() * self.dim);
        for e in embeddings {
            if e.len() != self.dim {
                return Err(ScanError::Dim { got: e.len(), want: self.dim });
            }
            flat.extend_from_slice(e);
        }
        check(unsafe { vrod_index_update(self.idx, ids.as_ptr(), flat.as_ptr(), ids.len() as u64) })
    }

    /// Physically removes the deleted rows (`ReindexCommand::execute`) and renumbers the survivors densely, in order.
    /// Returns the new id of every old row (`u64::MAX` for a deleted one); afterwards `len() == live_len()`.
    pub fn compact(&mut self) -> Result<Vec<u64>, ScanError> {
        let mut map = vec![0u64; self.len() as usize];
        check(unsafe { vrod_index_compact(self.idx, map.as_mut_ptr(), map.len() as u64) })?;
        Ok(map)
    }

    /// Rows added minus rows deleted.
    pub fn live_len(&self) -> u64 {
        let mut n = 0u64;
        unsafe { vrod_index_live_count(self.idx, &mut n) };
        n
    }

    /// Allow-list filter for every later search: `Some(allowed)` -- entry i true = id offset + i may be returned, rows
    /// past `allowed.len()` (rows added later included) may not -- or `None` to clear.  `allowed.len()` must not exceed
    /// `len()`.  Results are those of the same search over the rows that are live and allowed.
    pub fn set_filter(&mut self, allowed: Option<&[bool]>) -> Result<(), ScanError> {
        match allowed {
            None => check(unsafe { vrod_index_set_filter(self.idx, std::ptr::null(), 0) }),
            Some(a) => {
                let mut words = vec![0u32; a.len() / 32 + 1];
                for (i, &b) in a.iter().enumerate() {
                    if b {
                        words[i / 32] |= 1u32 << (i % 32);
                    }
                }
                check(unsafe { vrod_index_set_filter(self.idx, words.as_ptr(), a.len() as u64) })
            }
        }
    }

    /// Rows the next search may return: live and allowed (`live_len()` without a filter).
    pub fn filter_len(&self) -> u64 {
        let mut n = 0u64;
        unsafe { vrod_index_filter_count(self.idx, &mut n) };
        n
    }

    /// Best-first `(ids, scores)`, `queries.len() * k` each; slots past `filter_len()` are `(u64::MAX, NaN)`.
    pub fn search(&self, queries: &[Vec<f32>], k: usize) -> Result<(Vec<u64>, Vec<f32>), ScanError> {
        for q in queries {
            if q.len() != self.dim {
                return Err(ScanError::Dim { got: q.len(), want: self.dim });
            }
        }
        let flat: Vec<f32> = queries.iter().flatten().copied().collect();
        let mut ids = vec![0u64; queries.len() * k];
        let mut scores = vec![0f32; queries.len() * k];
        check(unsafe {
            vrod_search(self.idx, flat.as_ptr(), queries.len() as u32, k as u32, ids.as_mut_ptr(), scores.as_mut_ptr())
        })?;
        Ok((ids, scores))
    }
}

impl Collection {
    /// Give the rows with ids `first_id..first_id + labels.len()` their labels (every row carries 0 until set).
    pub fn set_labels(&mut self, first_id: u64, labels: &[u32]) -> Result<(), ScanError> {
        check(unsafe { vrod_index_set_labels(self.idx, first_id, labels.as_ptr(), labels.len() as u64) })
    }

    pub fn labels(&self, first_id: u64, n: usize) -> Result<Vec<u32>, ScanError> {
        let mut out = vec![0u32; n];
        check(unsafe { vrod_index_get_labels(self.idx, first_id, n as u64, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// `search` with a label per query: query `q` sees only the live, allowed rows labelled `labels[q]`.
    pub fn search_labeled(&self, queries: &[Vec<f32>], k: usize, labels: &[u32]) -> Result<(Vec<u64>, Vec<f32>), ScanError> {
        for q in queries {
            if q.len() != self.dim {
                return Err(ScanError::Dim { got: q.len(), want: self.dim });
            }
        }
        if labels.len() != queries.len() {
            return Err(ScanError::Dim { got: labels.len(), want: queries.len() });
        }
        let flat: Vec<f32> = queries.iter().flatten().copied().collect();
        let mut ids = vec![0u64; queries.len() * k];
        let mut scores = vec![0f32; queries.len() * k];
        check(unsafe {
            vrod_search_labeled(self.idx, flat.as_ptr(), queries.len() as u32, k as u32, labels.as_ptr(), ids.as_mut_ptr(), scores.as_mut_ptr())
        })?;
        Ok((ids, scores))
    }
}

impl Collection {
    /// Give the rows with ids `first_id..first_id + tags.len()` their 64-bit tag masks (every row carries 0 until set).
    pub fn set_tags(&mut self, first_id: u64, tags: &[u64]) -> Result<(), ScanError> {
        check(unsafe { vrod_index_set_tags(self.idx, first_id, tags.as_ptr(), tags.len() as u64) })
    }

    pub fn tags(&self, first_id: u64, n: usize) -> Result<Vec<u64>, ScanError> {
        let mut out = vec![0u64; n];
        check(unsafe { vrod_index_get_tags(self.idx, first_id, n as u64, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// `search` with a tag predicate per query: query `q` sees only the live, allowed rows whose tags match `preds[q]`.
    pub fn search_tagged(&self, queries: &[Vec<f32>], k: usize, preds: &[vrod_tag_pred]) -> Result<(Vec<u64>, Vec<f32>), ScanError> {
        for q in queries {
            if q.len() != self.dim {
                return Err(ScanError::Dim { got: q.len(), want: self.dim });
            }
        }
        if preds.len() != queries.len() {
            return Err(ScanError::Dim { got: preds.len(), want: queries.len() });
        }
        let flat: Vec<f32> = queries.iter().flatten().copied().collect();
        let mut ids = vec![0u64; queries.len() * k];
        let mut scores = vec![0f32; queries.len() * k];
        check(unsafe {
            vrod_search_tagged(self.idx, flat.as_ptr(), queries.len() as u32, k as u32, preds.as_ptr(), ids.as_mut_ptr(), scores.as_mut_ptr())
        })?;
        Ok((ids, scores))
    }

    /// Give the rows with ids `first_id..first_id + values.len()` their signed 64-bit values (every row carries 0 until set).
    pub fn set_values(&mut self, first_id: u64, values: &[i64]) -> Result<(), ScanError> {
        check(unsafe { vrod_index_set_values(self.idx, first_id, values.as_ptr(), values.len() as u64) })
    }

    pub fn values(&self, first_id: u64, n: usize) -> Result<Vec<i64>, ScanError> {
        let mut out = vec![0i64; n];
        check(unsafe { vrod_index_get_values(self.idx, first_id, n as u64, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// `search` with a tags + value-interval predicate per query: query `q` sees only the live, allowed rows whose tags
    /// and value match `preds[q]`.
    pub fn search_where(&self, queries: &[Vec<f32>], k: usize, preds: &[vrod_where]) -> Result<(Vec<u64>, Vec<f32>), ScanError> {
        for q in queries {
            if q.len() != self.dim {
                return Err(ScanError::Dim { got: q.len(), want: self.dim });
            }
        }
        if preds.len() != queries.len() {
            return Err(ScanError::Dim { got: preds.len(), want: queries.len() });
        }
        let flat: Vec<f32> = queries.iter().flatten().copied().collect();
        let mut ids = vec![0u64; queries.len() * k];
        let mut scores = vec![0f32; queries.len() * k];
        check(unsafe {
            vrod_search_where(self.idx, flat.as_ptr(), queries.len() as u32, k as u32, preds.as_ptr(), ids.as_mut_ptr(), scores.as_mut_ptr())
        })?;
        Ok((ids, scores))
    }
}

impl Collection {
    /// Give the rows with ids `first_id..first_id + keys.len()` the caller's keys (`u64::MAX`: no key).  No two live rows
    /// may hold the same key; a host that keys its payloads by them renumbers nothing after `compact`.
    pub fn set_keys(&mut self, first_id: u64, keys: &[u64]) -> Result<(), ScanError> {
        check(unsafe { vrod_index_set_keys(self.idx, first_id, keys.as_ptr(), keys.len() as u64) })
    }

    pub fn keys(&self, first_id: u64, n: usize) -> Result<Vec<u64>, ScanError> {
        let mut out = vec![u64::MAX; n];
        check(unsafe { vrod_index_get_keys(self.idx, first_id, n as u64, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// The id of the live row that holds each key, `u64::MAX` where none does.
    pub fn find_keys(&self, keys: &[u64]) -> Result<Vec<u64>, ScanError> {
        let mut out = vec![u64::MAX; keys.len()];
        check(unsafe { vrod_index_find_keys(self.idx, keys.as_ptr(), keys.len() as u64, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// The key each id's row stores (a search's ids -> the caller's names), `u64::MAX` where there is none.
    pub fn ids_to_keys(&self, ids: &[u64]) -> Result<Vec<u64>, ScanError> {
        let mut out = vec![u64::MAX; ids.len()];
        check(unsafe { vrod_index_ids_to_keys(self.idx, ids.as_ptr(), ids.len() as u64, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// Delete the live row of each key; unknown keys are ignored.  Returns the number of rows that died.
    pub fn delete_keys(&mut self, keys: &[u64]) -> Result<u64, ScanError> {
        let mut died = 0u64;
        check(unsafe { vrod_index_delete_keys(self.idx, keys.as_ptr(), keys.len() as u64, &mut died) })?;
        Ok(died)
    }

    /// Update the row of each key in place, or append it and give it the key.  Returns each key's id.
    pub fn upsert(&mut self, keys: &[u64], embeddings: &[Vec<f32>]) -> Result<Vec<u64>, ScanError> {
        if embeddings.len() != keys.len() {
            return Err(ScanError::Dim { got: embeddings.len(), want: keys.len() });
        }
        for e in embeddings {
            if e.len() != self.dim {
                return Err(ScanError::Dim { got: e.len(), want: self.dim });
            }
        }
        let flat: Vec<f32> = embeddings.iter().flatten().copied().collect();
        let mut ids = vec![u64::MAX; keys.len()];
        check(unsafe { vrod_index_upsert(self.idx, keys.as_ptr(), flat.as_ptr(), keys.len() as u64, ids.as_mut_ptr()) })?;
        Ok(ids)
    }

    pub fn key_stats(&self) -> Result<vrod_key_stats, ScanError> {
        let mut st = vrod_key_stats::default();
        check(unsafe { vrod_index_key_stats(self.idx, &mut st) })?;
        Ok(st)
    }
}

impl Collection {
    /// Every row at least as good as `thresholds[q]` (`>=` for cosine / inner product, `<=` for L2), best first:
    /// `(lims, ids, scores)` with query `q`'s rows at `lims[q]..lims[q + 1]`.  A count-only call sizes the buffers.
    pub fn range_search(&self, queries: &[Vec<f32>], thresholds: &[f32]) -> Result<(Vec<u64>, Vec<u64>, Vec<f32>), ScanError> {
        for q in queries {
            if q.len() != self.dim {
                return Err(ScanError::Dim { got: q.len(), want: self.dim });
            }
        }
        if thresholds.len() != queries.len() {
            return Err(ScanError::Dim { got: thresholds.len(), want: queries.len() });
        }
        let flat: Vec<f32> = queries.iter().flatten().copied().collect();
        let nq = queries.len() as u32;
        let mut lims = vec![0u64; queries.len() + 1];
        let rc = unsafe {
            vrod_range_search(self.idx, flat.as_ptr(), nq, thresholds.as_ptr(), 0, lims.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut())
        };
        if rc != VROD_ERR_CAPACITY {
            check(rc)?;
            return Ok((lims, Vec::new(), Vec::new()));
        }
        let n = lims[queries.len()] as usize;
        let mut ids = vec![0u64; n];
        let mut scores = vec![0f32; n];
        check(unsafe {
            vrod_range_search(self.idx, flat.as_ptr(), nq, thresholds.as_ptr(), n as u64, lims.as_mut_ptr(), ids.as_mut_ptr(), scores.as_mut_ptr())
        })?;
        Ok((lims, ids, scores))
    }
}

impl Drop for Collection {
    fn drop(&mut self) {
        unsafe { vrod_index_destroy(self.idx) };
    }
}

/// `f,f,...,f;word` -- the line format `write_embeddings_to_file` produces (`src/utils/embeddings.rs:55-61`).
pub fn parse_embedding_line(line: &str) -> Option<(Vec<f32>, &str)> {
    let (nums, word) = match line.find(';') {
        Some(i) => (&line[..i], &line[i + 1..]),
        None => (line, ""),
    };
    let v: Result<Vec<f32>, _> = nums.split(',').map(|t| t.trim().parse::<f32>()).collect();
    v.ok().filter(|v| !v.is_empty()).map(|v| (v, word))
}
