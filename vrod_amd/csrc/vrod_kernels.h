// vrod_kernels.h -- host-callable launchers of the HIP kernels (internal to libvrod_hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "search_plan.h"   // kSelectChunk
#include "label_plan.h"    // SegEntry
#include "tag_plan.h"      // TagPred
#include "where_plan.h"    // WherePred
#include "rowpred_plan.h"  // RowPred
#include "order_plan.h"    // OrderState
#include "aggregate_plan.h" // AggTable, AggGroup
#include "centroid_plan.h"  // the centroid scale and geometry
#include "multivec_plan.h" // MultivecQuery
#include "combine_plan.h"  // kCombineMaxExclude, combine_lanes_per_query
#include "candidates_plan.h" // kCandMaxList, the sort classes, cand_tile_query

namespace vrod {

// How a shard's local row index becomes the id the caller sees.  Single-device index: row + offset.
// Shard `shard` of a multi-device handle (rows dealt to `n_shards` shards in blocks of `block_rows`:
// global r -> shard (r / B) % G, local (r / (B*G)) * B + r % B):
//   id = ((row / B) * G + shard) * B + row % B + offset
// -- monotonic within a shard, so a list sorted by (score, local row) stays sorted by (score, id).
struct IdMap {
    uint64_t offset = 0;
    uint32_t block_rows = 0;   // 0: identity mapping
    uint32_t shard = 0, n_shards = 1;
    __host__ __device__ inline uint64_t operator()(uint32_t row) const {
        if (block_rows == 0) return (uint64_t)row + offset;
        const uint64_t b = row / block_rows, r = row % block_rows;
        return (b * n_shards + shard) * block_rows + r + offset;
    }
};

// ---- kernels_prep.hip
void launch_synth_rows(uint64_t seed, uint64_t first_row, uint64_t n, uint32_t dim, float* d_out,
                       hipStream_t s);
// Queries: normalise (COSINE) / round (BF16) / zero-pad to [nq_pad][ld] in ONE launch; also the
// fast squared norms qn2[nq_pad], the NaN/Inf flag and the max squared norm (float bits).
// `init`: per-search state the same launch resets (block q: status[q], counts[q], thr[q];
// block 0: n_zero_words words at zero_words) -- replaces five memset launches.
struct QueryInit {
    uint32_t* status;        // [nq_pad] -> 0
    uint32_t* counts;        // [nq_pad] -> 0 (may be null)
    float* thr;              // [nq_pad] -> thr_live_bits for q < nq, thr_pad_bits beyond (may be null)
    uint32_t thr_live_bits, thr_pad_bits;
    uint32_t* zero_words;    // scalars to clear (may be null)
    uint32_t n_zero_words;
    uint32_t* zero_words2;   // a second range (the pacing counters of the coming scan launches)
    uint32_t n_zero_words2;
};
// bf16 split of fp32 rows: corpus rows -> [hi | lo] (2*ldp), query rows -> [hi | hi | lo] (3*ldp)
void launch_split_rows(const float* d_in, uint64_t n, uint32_t ld, uint32_t ldp, void* d_out, bool queries, hipStream_t s);
void launch_prep_queries(const float* d_in, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t ld, int metric,
                         int dtype, float* d_out_f32, void* d_out_bf16, float* d_qn2, uint32_t* d_bad_flag,
                         uint32_t* d_max_bits, const QueryInit& init, hipStream_t s);
// tail of a search: status[nq] followed by {bad flag, max |q|^2 bits, max err bits, max |x|^2 bits}
// gathered into one contiguous block so that the host needs ONE device-to-host copy
void launch_gather_readback(const uint32_t* d_status, uint32_t nq, uint32_t* d_flags3, const uint32_t* d_max_xn2,
                            uint32_t* d_out, hipStream_t s);
void launch_row_fastnorm(const void* d_rows, int dtype, uint64_t n, uint32_t ld, float* d_xn2,
                         uint32_t* d_max_bits, hipStream_t s);

// ---- kernels_ingest.hip : THE prepare of rows -- the host forms' staged fp32 chunk (stride dim) and the _device forms'
// typed, strided rows alike.
// n typed rows (src_dtype: ingest_plan.h SRC_*), row r at element (d_pick ? d_pick[r] : r) * row_stride of d_src, become
// prepared rows [n][ld] at d_out (prep_chain.h's arithmetic on the values widened to fp32: COSINE normalises, a bf16
// handle rounds, the padding is zeroed), in one read of the source; NaN / Inf raise *d_bad_flag.
void launch_ingest_rows(const void* d_src, int src_dtype, uint64_t row_stride, const uint64_t* d_pick, uint64_t n, uint32_t dim,
                        uint32_t ld, int metric, int dtype, uint32_t* d_bad_flag, void* d_out, hipStream_t s);
// the same rows as dense rows [n][dim] of their own type (the staging leg of a source on another device)
void launch_ingest_pack(const void* d_src, int src_dtype, uint64_t row_stride, const uint64_t* d_pick, uint64_t n, uint32_t dim,
                        void* d_out, hipStream_t s);
// stored rows [n][ld] widened back to fp32, out_stride (>= dim) floats between the rows written
void launch_rows_get_strided(const void* d_rows, int dtype, uint64_t n, uint32_t dim, uint32_t ld, float* d_out, uint64_t out_stride,
                             hipStream_t s);

// ---- kernels_mutate.hip : vrod_index_update / vrod_index_compact
// Update: prepared row i of d_staged becomes corpus row d_dst[i] (kScatterSkip: left out), with its xnorm2 entry, the
// running maximum and -- fp32 handles, rows below planes_rows of non-null d_planes -- its bf16 [hi | lo] planes.
constexpr uint32_t kScatterSkip = 0xFFFFFFFFu;
void launch_scatter_rows(const void* d_staged, const uint32_t* d_dst, uint64_t n, int dtype, uint32_t ld, void* d_corpus,
                         float* d_xn2, uint32_t* d_max_bits, void* d_planes, uint64_t planes_rows, uint32_t ldp, hipStream_t s);
// Compact: the live rows of [r0, r1) (r0 % 32 == 0; d_del: the deleted-row bitmap; d_word_base: compact_plan.h
// compact_word_bases) move to d_out_rows / d_out_xn2 at their destination minus out_base.
void launch_compact_rows(const void* d_rows, const float* d_xn2, const uint32_t* d_del, const uint32_t* d_word_base, uint64_t r0,
                         uint64_t r1, size_t row_bytes, void* d_out_rows, float* d_out_xn2, uint64_t out_base, hipStream_t s);
// *d_max_bits (cleared by the caller) = max of d_xn2[0, n) as float bits
void launch_xn2_max(const float* d_xn2, uint64_t n, uint32_t* d_max_bits, hipStream_t s);

// ---- kernels_snapshot.hip : vrod_index_save / vrod_index_load
// Pack: n_rows stored rows (pitch ld) -> d_dense, [n_rows][dim] elements; unpack: the inverse (only the rows' elements are
// written).  Both add the checksum terms (snapshot_plan.h) of the dense words, the first of which has the section-wide
// index first_word, to *d_sum.  n_rows * dim * element size <= kSnapChunkBytesMax; d_dense holds that rounded up to 4.
void launch_snapshot_pack(const void* d_rows, uint64_t n_rows, uint32_t dim, uint32_t ld, int dtype, void* d_dense, uint64_t first_word,
                          uint64_t* d_sum, hipStream_t s);
void launch_snapshot_unpack(const void* d_dense, uint64_t n_rows, uint32_t dim, uint32_t ld, int dtype, void* d_rows, uint64_t first_word,
                            uint64_t* d_sum, hipStream_t s);
// *d_sum += the checksum terms of n_bytes at d_bytes (4-byte aligned)
void launch_snapshot_checksum(const void* d_bytes, uint64_t n_bytes, uint64_t first_word, uint64_t* d_sum, hipStream_t s);

// ---- kernels_keys.hip : the row keys' device table (keys_plan.h) and the id -> key gather
struct KeyTable {
    uint64_t* slot_key = nullptr;   // [slots], kKeyNone = empty
    uint32_t* slot_row = nullptr;   // [slots]
    uint64_t slots = 0;             // a power of two
};
// what a launch leaves for the host, cleared by the host in front of it
struct KeyCounters {
    unsigned long long claimed;     // insert / rebuild: slots newly claimed
    unsigned long long find_walk;   // find: slots visited, all keys together
    uint32_t max_probe;             // insert / rebuild: the longest walk, in slots
    uint32_t err;                   // kKeyErrFull | kKeyErrHeld
};
// d_col: the key column [count]; d_del: the deleted-row bits, or null while nothing was ever deleted.
// check: keys d_keys[0, n) are about to go to rows [r0, r0 + n).  insert: the column holds them already.
void launch_keys_check(const KeyTable& T, const uint64_t* d_col, const uint32_t* d_del, uint64_t count, const uint64_t* d_keys, uint64_t r0,
                       uint64_t n, KeyCounters* d_ctr, hipStream_t s);
void launch_keys_insert(const KeyTable& T, const uint64_t* d_col, const uint32_t* d_del, uint64_t r0, uint64_t n, bool rebuild,
                        KeyCounters* d_ctr, hipStream_t s);
void launch_keys_find(const KeyTable& T, const uint64_t* d_col, const uint32_t* d_del, uint64_t count, uint64_t id_offset,
                      const uint64_t* d_keys, uint64_t n, uint64_t* d_out_ids, KeyCounters* d_ctr, hipStream_t s);
void launch_keys_translate(const uint64_t* d_col, uint64_t count, uint64_t id_offset, const uint64_t* d_ids, uint64_t n, uint64_t* d_out_keys,
                           hipStream_t s);

// ---- kernels_stream.hip : Q <= 8 HBM-bound scan, writes fast scores [nq_pad][score_ld]
// nq_pad in {1,2,4,8}; d_q is [nq_pad][ld] prepared fp32 (zero rows for padding).
// Also accumulates, per query, a histogram of the top stream_hist_bits(nq_pad) bits of the
// score keys into d_hist [nq_pad][1 << bits] (must be zeroed by the caller): only the bins at
// or above each block's own kp-th best are published, which is all the global select needs.
// d_row_mask (may be null): bit r of word r / 32 set = row r is excluded (deleted): neither its score is written nor is
// it counted in the histogram (a separate kernel instantiation, launched only with a mask).
void launch_scan_stream(const void* d_corpus, int dtype, int metric, uint32_t ld, uint64_t nrows,
                        const float* d_q, int nq_pad, float* d_scores, uint64_t score_ld,
                        uint32_t* d_hist, uint32_t kp, const uint32_t* d_row_mask, hipStream_t s);
int stream_hist_bits(int nq_pad);
int stream_max_queries_per_pass(uint32_t ld);   // 8 .. 1 by LDS capacity, 0: the row does not fit
// Radix-select step 2: find the histogram bin holding the kp-th best score, then compact
// every row whose key falls in that bin or a better one into d_keys[q][...] (composite keys,
// unordered), counting into d_cnt[q].  More than `cap` such rows -> d_status[q] bit 1.  Rows set in d_row_mask (may be
// null) are never collected.
void launch_hist_compact(const float* d_scores, uint64_t score_ld, uint64_t n, int nq, int metric,
                         const uint32_t* d_hist, int hist_bits, uint32_t kp, uint64_t* d_keys,
                         uint32_t cap, uint32_t* d_cnt, uint32_t* d_status, const uint32_t* d_row_mask,
                         hipStream_t s);

// ---- kernels_select.hip
// Level 0: fast scores (implicit ids = column index) -> per-chunk top-kp composite keys.
// Later levels: keys -> keys.  Returns the number of keys per query written to d_out.
// chunk capacity is kSelectChunk (search_plan.h); kp <= kSelectChunk/2.  d_len (may be null; a labelled search): query q
// has only d_len[q] <= n columns, the rest of its score row is padding and never a key.  Level 0 leaves the rows set in d_row_mask
// (may be null) out: they become the empty key 0, which ranks below every row (a NaN score included) and is emitted as
// an unfilled slot.
uint64_t launch_select_from_scores(const float* d_scores, uint64_t score_ld, uint64_t n, int nq,
                                   int metric, uint32_t kp, uint64_t* d_out, uint64_t out_ld,
                                   const uint32_t* d_row_mask, hipStream_t s, const uint32_t* d_len = nullptr);
uint64_t launch_select_from_keys(const uint64_t* d_in, uint64_t in_ld, uint64_t n, int nq,
                                 uint32_t kp, uint64_t* d_out, uint64_t out_ld, hipStream_t s);
// Final step of a select chain: keys (n <= kSelectChunk per query, sorted or not) ->
// candidate rows [nq][kp] (sorted best first, ~0u padding) and T[q] = fast score of the
// kp-th candidate (worst score if fewer than kp candidates exist: nothing was left out).
// d_cnt != nullptr: the number of keys of query q is min(d_cnt[q], n) (device-side count).
void launch_keys_to_candidates(const uint64_t* d_keys, uint64_t key_ld, uint64_t n, int nq,
                               int metric, uint32_t kp, uint32_t* d_cand_rows, float* d_cand_fast,
                               float* d_T, const uint32_t* d_cnt, hipStream_t s);

// MFMA path: per-query candidate lists {fast score bits, row} appended by the scan kernel.
// Sort each list, keep the best `keep`, write thr[q] = keep-th fast score (worst if short),
// flag overflow (count > cap) in d_status[q] bit 1.
// A list shorter than `keep` leaves thr[q] unchanged (rows were still left out at that threshold).
// d_cand_rows != nullptr (last compaction of a search): also emit candidates [nq][keep]
// (rows, fast scores; ~0u / NaN padding) and T[q] = the threshold every left-out row fails.
void launch_list_compact(uint2* d_lists, uint32_t* d_counts, uint32_t cap, int nq, int metric,
                         uint32_t keep, float* d_thr, uint32_t* d_status, uint32_t* d_cand_rows,
                         float* d_cand_fast, float* d_T, hipStream_t s);
// Sample pass: thr[q] = the j-th best of the n_sample fast scores scores[q][0..n_sample)
// (exact, 3-pass radix select on the order-preserving key).  One block per query.
void launch_sample_select(const float* d_scores, uint64_t score_ld, uint32_t n_sample, int nq,
                          int metric, uint32_t j, float* d_thr, hipStream_t s);
// Dense sample block of a handle with deleted rows: column c of every query (c < n_sample) becomes the worst score when
// row row0 + c is set in d_row_mask, so that the sample's j-th best is that of live rows only.
void launch_mask_sample(float* d_scores, uint64_t score_ld, uint32_t n_sample, int nq, uint64_t row0,
                        const uint32_t* d_row_mask, int metric, hipStream_t s);
// Final: canonical scores of the kp candidates -> sorted top-k (ids u64 = idmap(row)),
// certificate per query in d_status bit 0 (1 = NOT certified).
// The certificate's bound on |fast - canonical| is formed on the device from the max squared
// norms (float bits) of the queries and of the corpus:  eps_mode 0: c * |q| * |x|  (dot paths),
// 1: c relative to T (direct L2),  2: c * (|q| + |x|)^2 (L2 through the norm expansion).
void launch_final_topk(const uint32_t* d_cand_rows, const float* d_cand_fast,
                       const float* d_cand_canon, const float* d_T, int nq, uint32_t kp, uint32_t k,
                       int metric, const IdMap& idmap, int eps_mode, float eps_c,
                       const uint32_t* d_max_qn2_bits, const uint32_t* d_max_xn2_bits,
                       uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_status,
                       float* d_max_err, hipStream_t s);

// Band pass (second chance of queries whose certificate failed; kernels_select.hip): thresholds c_k -/+ eps and
// reset counters for the nf failed queries (original indices d_qidx), their prepared rows gathered into a dense
// block, and the scatter of the resolved queries' results back to the caller's rows.
void launch_band_prepare(const uint32_t* d_qidx, uint32_t nf, uint32_t nf_pad, const float* d_out_scores, uint32_t k, int metric,
                         int eps_mode, float eps_c, const uint32_t* d_max_qn2_bits, const uint32_t* d_max_xn2_bits,
                         const float* d_qn2_all, float* d_thr, float* d_qn2, uint32_t* d_counts, uint32_t* d_ok, hipStream_t s);
void launch_gather_query_rows(const float* d_src, const uint32_t* d_qidx, uint32_t nf, uint32_t nf_pad, uint32_t ld, float* d_dst_f32,
                              void* d_dst_bf16, hipStream_t s);
void launch_scatter_results(const uint64_t* d_ids, const float* d_scores, const uint32_t* d_qidx, const uint32_t* d_resolved, uint32_t nf,
                            uint32_t k, uint64_t* d_out_ids, float* d_out_scores, hipStream_t s);

// Exact path: canonical scores (implicit ids) -> exact top-k, via the same select chain with
// composite keys (ties -> smaller id).  Writes one query's output row.
void launch_keys_to_output(const uint64_t* d_keys, uint64_t n, int metric, uint32_t k,
                           const IdMap& idmap, uint64_t* d_out_ids, float* d_out_scores,
                           hipStream_t s);
// Gather path output: the keys of nq queries (n per query, row stride key_ld) name columns of the ascending row list
// d_list; column c -> row d_list[c] -> idmap.  One launch for all nq queries, outputs [nq][k].
void launch_list_keys_to_output(const uint64_t* d_keys, uint64_t key_ld, uint64_t n, int nq, int metric, uint32_t k,
                                const uint32_t* d_list, const IdMap& idmap, uint64_t* d_out_ids, float* d_out_scores,
                                hipStream_t s);

// Labelled search output: as launch_list_keys_to_output, with a list segment (d_lists + d_seg_base[s]) and an output row
// (d_slot_q[s]) of its own per score slot s < ns.
void launch_seg_keys_to_output(const uint64_t* d_keys, uint64_t key_ld, uint64_t n, int ns, int metric, uint32_t k,
                               const uint32_t* d_lists, const uint32_t* d_seg_base, const uint32_t* d_slot_q, const IdMap& idmap,
                               uint64_t* d_out_ids, float* d_out_scores, hipStream_t s);

// Fill a result block with "no result" (ids = UINT64_MAX, scores = NaN): the empty list slots of
// the multi-device exchange.
void launch_fill_none(uint64_t* d_ids, float* d_scores, uint64_t n, hipStream_t s);
// Merge n_lists per-shard results into one. List l's ids start at d_ids + l*list_stride_ids
// (elements), its scores at d_scores + l*list_stride_scores; each is [nq][k].
void launch_merge_topk(int metric, const uint64_t* d_ids, const float* d_scores, uint64_t list_stride_ids,
                       uint64_t list_stride_scores, uint32_t n_lists, uint32_t nq, uint32_t k,
                       uint64_t* d_out_ids, float* d_out_scores, hipStream_t s);

// ---- kernels_rescore.hip : canonical (oracle-order) scores
// d_q: [nq][ld] prepared fp32.  Candidates: rows [nq][kp] (~0u = empty slot -> NaN score).
void launch_rescore_candidates(const void* d_corpus, int dtype, int metric, uint32_t dim,
                               uint32_t ld, const float* d_q, int nq, const uint32_t* d_cand_rows,
                               uint32_t kp, float* d_out, hipStream_t s);
// All rows of the shard for nq in {1, 2, 4, 8} queries in ONE pass over the corpus (the exact
// path): query n is row query_index[n] of d_q; out[n * out_ld + row].  nq must not exceed
// rescore_all_max_queries(ld) (LDS: nq query rows beside the staging tile).
int rescore_all_max_queries(uint32_t ld);
void launch_rescore_all(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld,
                        const float* d_q, const uint32_t* query_index, int nq, uint64_t nrows,
                        float* d_out, uint64_t out_ld, hipStream_t s);
// Gather path of a filtered search: canonical scores (the rescore_all chain) of the m rows d_list names (ascending local
// row indices) for nq consecutive prepared queries d_q [nq][ld]: d_out[q * out_ld + c] = score of row d_list[c].
// One launch serves any nq (queries in groups of 8 per lane, rows in tiles of 64 per wave).
void launch_rescore_list(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q, uint32_t nq,
                         const uint32_t* d_list, uint64_t m, float* d_out, uint64_t out_ld, hipStream_t s);

// Segmented form (a labelled search, label_plan.h): ONE launch of n_blocks blocks scores every entry of the work table
// d_entries -- per entry a group of queries (score slots; slot s is prepared row d_slot_q[s] of d_q) over its own
// segment of the row lists d_lists: d_out[(s - slot_first) * out_ld + c] = score of row d_lists[list_base + c].
void launch_rescore_segments(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q,
                             const SegEntry* d_entries, uint32_t n_entries, uint32_t n_blocks, const uint32_t* d_slot_q, uint32_t slot_first,
                             const uint32_t* d_lists, float* d_out, uint64_t out_ld, hipStream_t s);

// ---- kernels_label.hip : rows grouped by the labels of a batch, one label's dense-scan mask
// Pass 1: d_cnt[b * cnt_ld + g] (b < ceil(count / rows_per_block)) = the eligible rows (not set in d_mask, which may be
// null) of block b that carry d_table[g] (sorted distinct labels, g < G <= kLabelGroupsPerPass).  d_labels == null:
// every row carries label 0.  launch_group_prefix over the whole matrix follows.
void launch_label_group_count(const uint32_t* d_labels, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block,
                              const uint32_t* d_table, uint32_t G, uint32_t* d_cnt, uint32_t cnt_ld, hipStream_t s);
// Pass 2, over the prefixed counts: group g's rows, ascending, into d_lists[d_seg_off[g] ...] (kNoSegment: the group
// gets no list).  A sub-range of the pass's table (and d_cnt + its first group) is a table too: it is still sorted.
void launch_label_group_scatter(const uint32_t* d_labels, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block,
                                const uint32_t* d_table, uint32_t G, const uint32_t* d_cnt, uint32_t cnt_ld, const uint32_t* d_seg_off,
                                uint32_t* d_lists, hipStream_t s);
// d_out [n_words]: bit r set = row r is set in d_mask (may be null), carries another label than `label`, or r >= count.
void launch_label_group_mask(const uint32_t* d_labels, const uint32_t* d_mask, uint64_t count, uint64_t n_words, uint32_t label,
                             uint32_t* d_out, hipStream_t s);
// d_dst row i = d_src row d_idx[i] (rows of dim floats)
void launch_gather_rows(const float* d_src, const uint32_t* d_idx, uint32_t n, uint32_t dim, float* d_dst, hipStream_t s);

// The prefix pass on its own: d_cnt [n_blocks][G] -> exclusive prefix over the blocks per group, d_total[g] = the sum.
void launch_group_prefix(uint32_t* d_cnt, uint32_t n_blocks, uint32_t G, uint32_t* d_total, hipStream_t s);

// ---- kernels_pred.hip : rows grouped by the predicates of a batch over their side columns, one predicate's dense-scan mask
// The columns a kind of row carries and the predicate over them.  A null column: every row carries 0, at no load.
struct TagRows { using Pred = TagPred; const uint64_t* tags; };                                          // G <= kTagGroupsPerPass
struct WhereRows { using Pred = WherePred; const uint64_t* tags; const int64_t* vals; };                 // G <= kWhereGroupsPerPass
struct RowPredRows { using Pred = RowPred; const uint64_t* tags; const int64_t* vals; const uint32_t* labels; };   // G <= kRowPredsPerPass
// Pass 1: d_cnt[b * cnt_ld + g] (b < ceil(count / rows_per_block)) = the eligible rows (not set in d_mask, which may be
// null) of block b that match d_table[g], g < G.  A row counts towards every group it matches.  launch_group_prefix over
// the whole matrix follows.  (vrod_index_count_where: RowPredRows, kRowPredRowsPerGroup rows a block, d_mask its scope.)
template <typename Rows>
void launch_pred_group_count(Rows rows, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block, const typename Rows::Pred* d_table,
                             uint32_t G, uint32_t* d_cnt, uint32_t cnt_ld, hipStream_t s);
// Pass 2, over the prefixed counts: group g's rows, ascending, into d_lists[d_seg_off[g] ...] (kNoSegment: no list).
template <typename Rows>
void launch_pred_group_scatter(Rows rows, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block, const typename Rows::Pred* d_table,
                               uint32_t G, const uint32_t* d_cnt, uint32_t cnt_ld, const uint32_t* d_seg_off, uint32_t* d_lists, hipStream_t s);
// d_out [n_words]: bit r set = row r is set in d_mask (may be null), does not match p, or r >= count.
template <typename Rows>
void launch_pred_group_mask(Rows rows, const uint32_t* d_mask, uint64_t count, uint64_t n_words, const typename Rows::Pred& p, uint32_t* d_out,
                            hipStream_t s);

// ---- kernels_rowpred.hip : a predicate over tags, value and label as an operation on the rows (vrod_index_*_where)
// Every pass gives work-group b rows [b * kRowPredRowsPerGroup, ...): row_pred_groups(count) groups.  A null column:
// every row carries 0.  d_scope (may be null): bit set = the row is out of scope.
// d_hits [row_pred_hit_words(count)]: bit r set = row r < count is in scope and matches p; d_cnt[b] (may be null) = the
// bits of group b.
void launch_rowpred_hits(const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope, uint64_t count,
                         const RowPred& p, uint32_t* d_hits, uint32_t* d_cnt, hipStream_t s);
// ... and whose tags t differ from t' = (t & ~clear_bits) | set_bits, which the row then carries.  d_tags is not null.
void launch_rowpred_retag(uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope, uint64_t count,
                          const RowPred& p, uint64_t set_bits, uint64_t clear_bits, uint32_t* d_hits, hipStream_t s);
// d_out[d_first[b] + j] = id_offset + the row of the j-th bit set in group b's words of d_hits (d_first: the prefixed
// counts): the selection in ascending order.
void launch_rowpred_scatter(const uint32_t* d_hits, uint64_t count, const uint32_t* d_first, uint64_t id_offset, uint64_t* d_out, hipStream_t s);

// ---- kernels_order.hip : the top rows by (value, id) under a row predicate and after a cursor (vrod_index_select_ordered)
// The geometry, columns and scope of kernels_rowpred.hip; keys, cursor test and state as order_plan.h defines them.
// d_hits / d_cnt as launch_rowpred_hits, a hit also lying strictly after (ckey, cid) when has_cursor; d_cnt is not null.
void launch_order_hits(const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope, uint64_t count,
                       const RowPred& p, bool desc, bool has_cursor, uint64_t ckey, uint64_t cid, uint64_t id_offset, uint32_t* d_hits,
                       uint32_t* d_cnt, hipStream_t s);
// The key of rank `limit` (1 <= limit <= the hit rows) among the hit rows, into *d_state: its pivot, and in `remaining`
// how many rows of the pivot's tie class the limit still takes.  d_hist [kOrderRounds][kOrderBins] is scratch.
void launch_order_select(const uint32_t* d_hits, const int64_t* d_vals, uint64_t count, bool desc, uint32_t limit, uint32_t* d_hist,
                         OrderState* d_state, hipStream_t s);
// The n_rec {key, id} records of the rows a call takes, in no particular order, into d_rec.  take_all: every hit row, group b
// from position d_first[b] (the prefixed counts of launch_order_hits).  Otherwise what *d_state says: d_cnt2
// [2 * groups + 2] is scratch.
void launch_order_collect(const uint32_t* d_hits, const int64_t* d_vals, uint64_t count, bool desc, uint64_t id_offset, bool take_all,
                          const OrderState* d_state, uint32_t* d_cnt2, const uint32_t* d_first, uint64_t* d_rec, uint32_t n_rec, hipStream_t s);
// d_rec (order_sort_size(n) records of room, the first n filled) sorted by (key, id); then d_out_ids[i] and d_out_vals[i]
// (may be null) = the id and the value of record i < n.
void launch_order_sort(uint64_t* d_rec, uint32_t n, bool desc, uint64_t* d_out_ids, int64_t* d_out_vals, hipStream_t s);

// ---- kernels_aggregate.hip : count, min / max / sum of the value and the smallest id per group (vrod_index_aggregate_where)
// The geometry, columns and scope of kernels_rowpred.hip; keys, tables and counters as aggregate_plan.h defines them.
// Every slot of g (slots + 1 of them) to the aggregates' identities and the counters to zero; direct (BY_TAG): slot i
// holds key i, otherwise every key word is empty.  Enqueued before the pass: no claimer initialises a slot.
void launch_agg_reset(const AggTable& g, bool direct, hipStream_t s);
// The rows in scope (d_scope as launch_rowpred_hits) that match p, aggregated into g by the key of mode `by`
// (kAggBy*; width: BY_VALUE's bucket); g.ctr->rows += their number.  A null column reads 0: pass only what p and `by` need.
void launch_agg_pass(uint32_t by, const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope,
                     uint64_t count, const RowPred& p, int64_t width, uint64_t id_offset, const AggTable& g, hipStream_t s);
// The occupied slots of g as records d_out[0 .. min(n, cap)) in no particular order, g.ctr->n_out = n.  d_out null: n only.
void launch_agg_compact(const AggTable& g, AggGroup* d_out, uint64_t cap, hipStream_t s);

// ---- kernels_centroid.hip : the exact vector sum or mean of every group (vrod_index_centroids_where)
// The groups are those of an aggregation pass that has ended (g, BY_LABEL or BY_VALUE), the rows those of a hit bitmap
// launch_rowpred_hits wrote for `count` rows; the arithmetic is centroid_plan.h's.
// d_rank[the slot of d_keys[i] in g] = i, i < n_groups; the other entries of d_rank [g.slots + 1] are left alone.
void launch_centroid_ranks(const AggTable& g, const int64_t* d_keys, uint32_t n_groups, uint32_t* d_rank, hipStream_t s);
// *d_max_bits = max(*d_max_bits, bits(x) & 0x7fffffff) over the elements below dim of the rows with their hit bit set.
void launch_centroid_max(const void* d_corpus, int dtype, uint32_t dim, uint32_t ld, const uint32_t* d_hits, uint64_t count, uint32_t* d_max_bits,
                         hipStream_t s);
// d_acc[rank of the row's key][j] += centroid_quantise(x, scale) for the same rows and elements, by 64-bit integer atomics:
// d_acc [n_groups][dim] starts at zero.  A null column reads 0, as in launch_agg_pass; `by`, width: that pass's.
void launch_centroid_add(const void* d_corpus, int dtype, uint32_t dim, uint32_t ld, const uint32_t* d_hits, uint64_t count, uint32_t by,
                         const int64_t* d_vals, const uint32_t* d_labels, int64_t width, const AggTable& g, const uint32_t* d_rank,
                         uint32_t n_groups, int32_t scale, int64_t* d_acc, hipStream_t s);
// d_out[g * stride + j] = the sum (sums) or the mean over d_counts[g] rows of d_acc[g][j] as fp32, j < dim.
void launch_centroid_finish(const int64_t* d_acc, const uint64_t* d_counts, uint32_t n_groups, uint32_t dim, int32_t scale, bool sums, float* d_out,
                            uint64_t stride, hipStream_t s);

// ---- kernels_dup.hip : the classes of live rows with the same stored bits (vrod_index_find_duplicates, _delete_duplicates)
// The table of one call (dup_plan.h): slot_row / slot_min [slots], all-ones before the class pass; row_slot [count].
struct DupTable {
    uint32_t* slot_row = nullptr;   // the row that claimed the slot, kDupEmpty = none
    uint32_t* slot_min = nullptr;   // the smallest row of the slot's class
    uint32_t* row_slot = nullptr;   // [count]: the slot of every live row
    uint64_t slots = 0;             // a power of two
};
// what the passes leave for the host, cleared by the host in front of them
struct DupCounters {
    unsigned long long classes;          // output: live rows that are their class's first
    unsigned long long compare_misses;   // class: full comparisons that found a difference
    uint32_t largest_class;              // output
    uint32_t max_probe;                  // class: the longest walk, in slots
    uint32_t err;                        // kDupErrFull | kDupErrSlot
    uint32_t pad;
};
// d_hash[r] = the hash (dup_plan.h dup_row_hash; within: the row's label mixed in, d_labels null: label 0) of every row
// r < count not set in d_del (may be null).  The corpus is read once, nothing else of it is touched.
void launch_dup_hash(const void* d_corpus, uint32_t dim, uint32_t ld, uint32_t esize, uint64_t count, const uint32_t* d_del, const uint32_t* d_labels,
                     bool within, bool narrow, uint64_t* d_hash, hipStream_t s);
// Every live row finds or claims the slot of its class: T.row_slot, T.slot_min; *d_ctr (zero before) gets the diagnostics.
void launch_dup_class(const void* d_corpus, uint32_t dim, uint32_t ld, uint32_t esize, uint64_t count, const uint32_t* d_del, const uint32_t* d_labels,
                      bool within, const uint64_t* d_hash, const DupTable& T, DupCounters* d_ctr, hipStream_t s);
// d_out_first [count] (may be null) = id_offset + the smallest row of the row's class, all-ones for a deleted row;
// d_class_size [count] is zero before; d_hits (may be null; row_pred_hit_words(count) words): bit r set = row r is live
// and not the first of its class.  Nothing is written when *d_ctr carries an error.
void launch_dup_output(uint64_t count, const uint32_t* d_del, const DupTable& T, uint64_t id_offset, uint64_t* d_out_first, uint32_t* d_class_size,
                       uint32_t* d_hits, DupCounters* d_ctr, hipStream_t s);

// ---- kernels_rowfind.hip : the join between a batch of prepared inputs and the corpus (vrod_index_find_rows, _add_unique)
struct RowfindAnswer;   // rowfind_plan.h: what the device says of one input
// d_stage [m][ld]: the batch's prepared rows, d_stage_hash [m] their hashes, T their class table (launch_dup_class over
// them).  d_found [T.slots] (all-ones before) gets, per class, the smallest row r < count of d_corpus that is not set in
// d_del (may be null) and whose dim stored elements equal the class's; d_hash [count]: the corpus rows' hashes, read for
// live rows only.  *d_ctr gets compare_misses, max_probe and err as the class pass's.
void launch_rowfind_probe(const void* d_corpus, uint32_t dim, uint32_t ld, uint32_t esize, uint64_t count, const uint32_t* d_del, const uint64_t* d_hash,
                          const void* d_stage, uint32_t m, const uint64_t* d_stage_hash, const DupTable& T, uint32_t* d_found, DupCounters* d_ctr,
                          hipStream_t s);
// d_ans [m]: per input its class's found row -- d_found's, else count0 + d_found_side's (may be null), else none -- and
// its first input of the batch.  Nothing is written when *d_ctr carries an error.
void launch_rowfind_resolve(uint32_t m, const DupTable& T, const uint32_t* d_found, const uint32_t* d_found_side, uint64_t count0, RowfindAnswer* d_ans,
                            const DupCounters* d_ctr, hipStream_t s);
// The batch's new inputs d_news [k] (indices into the batch): d_dst_hash [k] = their hashes, d_dst_rows [k][ld] (may be
// null) = their staged rows.
void launch_rowfind_keep(const void* d_stage, uint32_t ld, uint32_t esize, const uint64_t* d_stage_hash, const uint32_t* d_news, uint32_t k,
                         void* d_dst_rows, uint64_t* d_dst_hash, hipStream_t s);

// ---- kernels_near.hip : the connected components of the threshold graph (vrod_index_find_near_duplicates, _delete_near_duplicates)
struct RangeHit;   // kernels_range.h: one qualifying (query, row) of a range search
// what the passes leave for the host, cleared by the host in front of the first union pass
struct NearCounters {
    unsigned long long hits;     // union: pool entries whose two rows differ (directed pairs)
    unsigned long long classes;  // flatten: eligible rows that are their component's root
    unsigned long long rows;     // flatten: eligible rows
    uint32_t largest_class;      // flatten
    uint32_t err;                // near_plan.h kNearErrWalk | kNearErrRetry | kNearErrRow
};
// d_parent[r] = r, d_class_size[r] = 0 for every r < count: every row a component of its own.
void launch_near_init(uint32_t* d_parent, uint32_t* d_class_size, uint64_t count, hipStream_t s);
// The `stored` entries of a range pool (unsorted) whose queries were rows d_batch_rows[0 .. batch_n) of the handle: entry
// {key, id} joins row d_batch_rows[key >> 32] and row id - id_offset in d_parent [count] (lock-free union-find, roots are
// minima); an entry whose two rows are one is skipped and not counted in d_ctr->hits.
void launch_near_union(const RangeHit* d_hits, uint64_t stored, const uint32_t* d_batch_rows, uint32_t batch_n, uint64_t id_offset, uint64_t count,
                       uint32_t* d_parent, NearCounters* d_ctr, hipStream_t s);
// d_out_first [count] (may be null) = id_offset + the root of the row's component, all-ones for a row set in d_mask (may
// be null: every row is eligible); d_class_size [count] is zero before; d_hits (may be null; row_pred_hit_words(count)
// words): bit r set = row r is eligible and not its component's root.  Nothing is written when *d_ctr carries an error.
void launch_near_flatten(uint64_t count, const uint32_t* d_mask, uint32_t* d_parent, uint64_t id_offset, uint64_t* d_out_first, uint32_t* d_class_size,
                         uint32_t* d_hits, NearCounters* d_ctr, hipStream_t s);

// ---- kernels_group.hip : a grouped search's de-duplication by label and the dense stage's per-query masks
// List b (d_cand_ids / d_cand_scores + b * k1: a search's result row, ids with id_offset applied) of query d_qidx[b] (b
// itself when d_qidx is null): the first entry of every label that is not among the d_found[q] < k results already in
// the query's row of d_out_* [..][k] is appended to them, in list order, while the row has room; d_found[q] = the new
// count, d_valid[q] = the list's real entries.  d_labels == null: every row carries label 0.  k1 <= kGroupMaxK.
void launch_group_dedupe(const uint64_t* d_cand_ids, const float* d_cand_scores, uint32_t k1, uint32_t n_lists, const uint32_t* d_labels,
                         uint64_t id_offset, const uint32_t* d_qidx, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                         uint32_t* d_out_labels, uint32_t* d_found, uint32_t* d_valid, hipStream_t s);
// d_out [n_queries][n_words]: bit r of row a set = row r is set in d_base_mask (may be null), carries one of the
// d_found[q] labels in d_out_labels [..][k] of q = d_qidx[a], or r >= count.  Written for the rows below count rounded up
// to 256, which must lie within n_words * 32 and within the label array.
void launch_group_mask(const uint32_t* d_labels, const uint32_t* d_base_mask, uint64_t count, uint64_t n_words, const uint32_t* d_qidx,
                       uint32_t n_queries, const uint32_t* d_out_labels, const uint32_t* d_found, uint32_t k, uint32_t* d_out, hipStream_t s);

// ---- kernels_multivec.hip : a multi-vector search's document scores (vrod_search_multivec)
// Dense route.  Fold: canonical scores d_scores [g][score_ld] of rows [0, n_rows) -> d_best [g][n_docs] (zeroed by the
// caller), the best score per (vector, document) as an order-preserving key; d_rank[r] = the document of row r (null: one
// document), rows set in d_mask (may be null) are left out.  Sum: d_S[d] = (first ? +0 : d_S[d]) + M(0, d) + ... in
// order; d_absent (may be null; ceil(n_docs / 32) words) = the bitmap of the documents without an eligible row.
void launch_multivec_fold(const float* d_scores, uint64_t score_ld, uint32_t g, uint64_t n_rows, const uint32_t* d_rank, const uint32_t* d_mask,
                          int metric, uint32_t* d_best, uint64_t n_docs, hipStream_t s);
void launch_multivec_sum(const uint32_t* d_best, uint32_t g, uint64_t n_docs, int metric, bool first, float* d_S, uint32_t* d_absent,
                         hipStream_t s);
// Candidate route.  Per query of d_queries (multivec_plan.h MultivecQuery) over the lists d_ids / d_scores [vectors][k1]:
// its distinct labels (unordered) at d_cand + ent_off, their number, flags (1: a short list, 2: a non-finite score) and U.
// d_lab: as many words as list entries; d_table: the queries' tables, all 0xFFFFFFFF.  d_labels == null: label 0.
void launch_multivec_candidates(const uint64_t* d_ids, const float* d_scores, uint32_t k1, const uint32_t* d_labels, uint64_t id_offset,
                                const MultivecQuery* d_queries, uint32_t nq, uint32_t* d_lab, uint32_t* d_table, uint32_t* d_cand, uint32_t* d_count,
                                uint32_t* d_flags, float* d_U, hipStream_t s);
// d_M[s] = the best of the first d_len[s] scores of slot s < n_slots of a score chunk [n_slots][score_ld] (NaN loses).
void launch_multivec_slot_best(const float* d_scores, uint64_t score_ld, uint32_t n_slots, const uint32_t* d_len, int metric, float* d_M,
                               hipStream_t s);
// d_out[d_dst[p]] = d_M[d_slot[p]] + ... + d_M[d_slot[p] + d_m[p] - 1], from +0, left to right.
void launch_multivec_pair_sum(const float* d_M, const uint32_t* d_slot, const uint32_t* d_m, const uint64_t* d_dst, uint32_t n_pairs, float* d_out,
                              hipStream_t s);
// Sorted keys [n_rows][key_ld] (kp per row, best first, 0 = none) over columns of d_table + d_tab_off[i] -> rows d_qidx[i]
// (i without d_qidx) of d_out_labels / d_out_scores [..][k], d_found[q] = filled slots, d_kth[i] (may be null) = slot k - 1.
void launch_multivec_output(const uint64_t* d_keys, uint64_t key_ld, uint32_t kp, uint32_t n_rows, int metric, uint32_t k, const uint32_t* d_table,
                            const uint32_t* d_tab_off, const uint32_t* d_qidx, uint32_t* d_out_labels, float* d_out_scores, uint32_t* d_found,
                            float* d_kth, hipStream_t s);

// ---- kernels_diverse.hip : the greedy selection of a diversified search (vrod_search_diverse)
// The search's lists d_list_ids / d_list_scores [nq][pool] (filled slots first, ids with id_offset applied) -> per query
// min(k, filled) rows by exact greedy MMR in selection order: d_out_ids / d_out_scores [nq][k], and v at the moment of
// selection in d_out_mmr (may be null); the slots no step fills are (~0, NaN, NaN).  mu = fl(1 - lambda) is taken here.
// One work-group per query; pool <= kDiverseMaxPool, dim <= kDiverseMaxDim (diverse_plan.h sizes the work-group).
void launch_diverse_select(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const uint64_t* d_list_ids,
                           const float* d_list_scores, uint32_t nq, uint32_t pool, uint32_t k, float lambda, uint64_t id_offset,
                           uint64_t* d_out_ids, float* d_out_scores, float* d_out_mmr, hipStream_t s);

// ---- kernels_byid.hip : queries taken from stored rows (vrod_search_by_ids, vrod_knn_graph)
// Rows [row0, row0 + m) against the deleted-row bitmap d_del (not null): d_live[j] = the j-th live row, ascending;
// d_src[i] = j for the live row row0 + i, ~0u for a deleted one.  One work-group: m is a batch.
void launch_byid_live(const uint32_t* d_del, uint64_t row0, uint32_t m, uint32_t* d_live, uint32_t* d_src, hipStream_t s);
// d_out [nq][dim] fp32 = the prepared rows as stored (bf16 widened), read with the handle's row stride ld.  Query q is
//   d_ids != null: row d_ids[q] - id_offset; an id that is no current row, or is set in d_del (may be null), raises
//                  *d_bad_flag and gives a zero row;
//   else d_rows != null: row d_rows[q];  else: row base_row + q  (a row >= count raises the flag as well).
// d_bad_flag may be null when the host has checked the rows already.
void launch_byid_gather(const void* d_corpus, int dtype, uint32_t ld, uint32_t dim, uint64_t count, uint64_t id_offset,
                        const uint32_t* d_del, const uint64_t* d_ids, const uint32_t* d_rows, uint64_t base_row, uint32_t nq, float* d_out,
                        uint32_t* d_bad_flag, hipStream_t s);
// Output row i < n_out [k] = result list d_src[i] (i when d_src is null; ~0u: an unfilled row) of d_list_* [..][k1], k1 >
// k, without the entry whose id is d_self[i] (base_id + i when d_self is null), cut to k.
void launch_byid_drop_self(const uint64_t* d_list_ids, const float* d_list_scores, uint32_t k1, const uint32_t* d_src, const uint64_t* d_self,
                           uint64_t base_id, uint32_t n_out, uint32_t k, uint64_t* d_out_ids, float* d_out_scores, hipStream_t s);

// ---- kernels_combine.hip : queries combined from stored rows, results minus an id set (vrod_search_combined)
// d_out [nq][dim] fp32: per coordinate +0, then acc = fl(acc + fl(w * x)) over query q's operands in order -- row q of d_vec
// ([nq][ld] prepared fp32; null: no vector operand) with weight d_vec_w[q] (null: 1), then the prepared stored rows
// d_term_ids[d_term_lims[q] .. d_term_lims[q + 1]) - id_offset as stored (bf16 widened) with weights d_term_w.  *d_flag
// gets kCombineBadId for a term id that is no current row or is set in d_del (may be null), kCombineBadWeight for a NaN /
// Inf weight, kCombineNonFinite for a NaN / Inf result.
constexpr uint32_t kCombineBadId = 1u, kCombineBadWeight = 2u, kCombineNonFinite = 4u;
void launch_combine_queries(const void* d_corpus, int dtype, uint32_t ld, uint32_t dim, uint64_t count, uint64_t id_offset, const uint32_t* d_del,
                            const float* d_vec, const float* d_vec_w, const uint32_t* d_term_lims, const uint64_t* d_term_ids,
                            const float* d_term_w, uint32_t nq, float* d_out, uint32_t* d_flag, hipStream_t s);
// Output row q [k] = row q of d_list_* [nq][k1] without the entries whose id is among d_excl_ids[d_excl_lims[q] ..
// d_excl_lims[q + 1]) (d_excl_lims null: none) or d_term_ids[d_term_lims[q] .. d_term_lims[q + 1]) (d_term_lims null:
// none), in order, cut to k and padded unfilled.  At most kCombineMaxExclude ids per query in all.
void launch_drop_excluded(const uint64_t* d_list_ids, const float* d_list_scores, uint32_t k1, const uint32_t* d_excl_lims,
                          const uint64_t* d_excl_ids, const uint32_t* d_term_lims, const uint64_t* d_term_ids, uint32_t nq, uint32_t k,
                          uint64_t* d_out_ids, float* d_out_scores, hipStream_t s);

// ---- kernels_candidates.hip : per-query id lists -> row segments, and their scores in list order (vrod_search_candidates,
// vrod_score_candidates)
// d_rows[i] = the local row of d_ids[i] (ids with id_offset applied), or kCandNoRow when the id is VROD_ID_NONE, no
// current row, or set in d_row_mask (may be null).
void launch_cand_resolve(const uint64_t* d_ids, uint32_t n, uint64_t count, uint64_t id_offset, const uint32_t* d_row_mask, uint32_t* d_rows,
                         hipStream_t s);
// One work-group per query q = d_qidx[b], b < n_queries, all of sort class `sort_class` (candidates_plan.h): the distinct
// rows of d_rows[d_lims[q] .. d_lims[q + 1]) without kCandNoRow, ascending, into d_lists from d_lims[q] on; d_len[q] =
// their number.
void launch_cand_sort_unique(const uint32_t* d_rows, const uint32_t* d_lims, const uint32_t* d_qidx, uint32_t n_queries, uint32_t sort_class,
                             uint32_t* d_lists, uint32_t* d_len, hipStream_t s);
// d_out[t] = the canonical score (the chain of rescore_chain.h, as a search reports it) of prepared query q of d_q [nq][ld]
// against row d_rows[t] for every t in [d_lims[q], d_lims[q + 1]); NaN where d_rows[t] is kCandNoRow.  d_tile_off [nq + 1]:
// cand_tile_offsets, n_tiles its last entry.  d_n_scored[q] (cleared by the caller) += the entries of q that were scored.
void launch_cand_score(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q, const uint32_t* d_lims,
                       const uint32_t* d_tile_off, uint32_t nq, uint32_t n_tiles, const uint32_t* d_rows, float* d_out, uint32_t* d_n_scored,
                       hipStream_t s);

// ---- kernels_mfma.hip : batched Q.K^T scan with fused threshold filter
// Timing of the dominant scan launches without marker packets: the launcher of the next scan
// kernel attaches these events to the dispatch itself (hipExtLaunchKernelGGL), then clears them.
// A marker recorded on the stream costs ~5 us of serialisation on each side of the kernel.
struct LaunchEvents { hipEvent_t start = nullptr, stop = nullptr; };
inline thread_local LaunchEvents g_launch_events;

struct MfmaScanArgs {
    const void* corpus;     // [capacity][ld] bf16 or f32
    const void* queries;    // [nq_pad][ld] same dtype (nq_pad multiple of 256)
    const float* xnorm2;    // [capacity] fast squared norms (L2 only)
    const float* qnorm2;    // [nq_pad] fast squared query norms (L2 only)
    const float* thr;       // [nq_pad] fast-score thresholds (append when strictly better)
    uint2* lists;           // [nq_pad][cap] {score bits, row}
    uint32_t* counts;       // [nq_pad]
    uint32_t cap;
    uint32_t ld;            // elements per row (multiple of 64 bf16 / 32 f32): the K extent, and the query row stride
    uint32_t lda_bytes;     // split-bf16 pass over fp32 rows (bf16 4-wave kernel, a_wrap != 0): the corpus row
    uint32_t a_wrap;        // stride in bytes ([hi_j | lo_j] planes; the query rows are [hi_j | lo_j | hi_j])
    uint32_t nq_pad;
    uint32_t nq;            // real queries (<= nq_pad): batches of <= 64 over bf16 rows take the skinny kernel
    uint32_t row_begin;     // appends are limited to rows [row_begin, row_end); the launch
    uint32_t row_end;       // starts at the 256-row tile containing row_begin
    int metric;
    uint32_t* pace;         // >= 128 words for the sibling pacing counters (may be null)
    bool pace_is_zero;      // the caller already cleared them (else the launcher issues a memset)
    float* dense_out;       // non-null: sample pass, write every fast score [nq_pad][dense_ld]
    uint32_t dense_ld;      // (column = row - row_begin; multiple of 256)
    bool dense_grouped;     // sample pass, grouped form: dense_out is [nq_pad][dense_ld] with ONE score per group of
                            // mfma_dense_group_rows() consecutive rows (the group's best), dense_ld = groups per query
    void* dump;             // mfma_dump_bytes(num_cus) bytes of scratch: where the 4-wave kernel spills full hit logs (filtered launches)
    uint32_t* claims;       // kMfmaClaimWords words: claim bits of the 4-wave kernel's work stealing for THIS launch; null: off
    bool claims_is_zero;    // the caller already cleared them (else the launcher issues a memset)
    const uint32_t* row_mask;   // filtered launches: bit r of word r / 32 set = row r is never appended (deleted); null: none
};
void launch_scan_mfma(const MfmaScanArgs& a, int dtype, int num_cus, hipStream_t s);

// Experiment switches (VROD_DEBUG_*): parsed ONCE per process, here and nowhere else (debug_env() in vrod_index.hip).
// The defaults are what every measurement in DESIGN.md was taken with; they exist for A/B runs (scripts/env_sweep.sh),
// not as a product surface -- the three variables a user may set are documented in include/vrod.h.
struct DebugEnv {
    int pace_kt = 192;            // VROD_DEBUG_PACE_KT: sibling pacing interval of the 4-wave scan, K-tiles (0: off)
    int pace_tiles = 16;          // VROD_DEBUG_PACE: ... of the 8-wave fp32 scan, tiles (0: off)
    bool w4_steal = true;         // VROD_DEBUG_W4_STEAL=0: static shares, no work stealing
    bool skinny = true;           // VROD_DEBUG_SKINNY=0: batches of 5-64 queries take the 256-query tile
    uint64_t stage_growth = 0;    // VROD_DEBUG_STAGE_GROWTH: rows grow x g per filtered stage (0: the default, 5)
    uint64_t sample_rows = 0;     // VROD_DEBUG_SAMPLE_ROWS: cap on the sample pass's rows (0: none)
    uint32_t kp_margin = 0;       // VROD_DEBUG_KP_MARGIN: starting candidate margin k' - k of the batched cosine scan (0: 8)
    int early_sample = -1;        // VROD_DEBUG_EARLY_SAMPLE=0 / 1: order of the two searches in flight (-1: by corpus size)
    bool sample_grouped = true;   // VROD_DEBUG_SAMPLE_GROUPED=0: the sample pass writes every score
    bool graph = true;            // VROD_DEBUG_GRAPH=0: no hipGraph replay of small searches
    bool band = true;             // VROD_DEBUG_BAND=0: failed certificates go straight to the exact path
};
const DebugEnv& debug_env();
size_t mfma_dump_bytes(int num_cus);
constexpr size_t kMfmaClaimWords = 256;    // >= query blocks per launch x strips (8 x work-groups per XCD in all)
// Rows per group of the grouped sample form for this launch (32), or 0 when the kernel that would take it only
// writes every score (dense_grouped must then stay false).
uint32_t mfma_dense_group_rows(const MfmaScanArgs& a, int dtype);
// Largest batch the skinny (HBM-bound, <= 64 queries) form of the MFMA scan takes for bf16 rows of
// `row_bytes` bytes (split == true: the [hi | lo] planes of an fp32 corpus); 0 = none.
uint32_t mfma_skinny_max_queries(bool split, uint32_t row_bytes);

}  // namespace vrod
