// kernels_range.h -- launchers of the range search's kernels (kernels_range.hip; internal to libvrod_hip).
#pragma once
#include "vrod_kernels.h"

namespace vrod {

// One qualifying (query, row) of a range search.  Ascending (key, id) order IS the result order: query ascending, then
// score best first (the low word of `key` is the complement of the order-preserving score key), then id ascending.
struct __attribute__((aligned(16))) RangeHit {
    uint64_t key;   // query << 32 | ~score_key(canonical score)
    uint64_t id;    // the id the caller sees (IdMap applied)
};

// Where the qualifying rows of a shard go.  `pool` holds `capacity` entries; n_total and per_query[q] keep counting
// when it is full, which is what makes the counts exact whatever the capacity is.
struct RangePool {
    RangeHit* pool;
    uint64_t capacity;
    unsigned long long* n_total;   // device scalar
    uint32_t* per_query;           // [nq]
};

// Per query: the fast-pass threshold (search_plan.h range_fast_threshold, formed from the batch's largest |q|^2 and the
// corpus's largest |x|^2 on the device) and canonical[q] = 1 when the query has no finite bound and must take the
// canonical route.  Padding queries q >= nq get a threshold nothing passes.
void launch_range_prepare(const float* d_thresholds, uint32_t nq, uint32_t nq_pad, int metric, int eps_mode, float eps_c,
                          const uint32_t* d_max_qn2_bits, const uint32_t* d_max_xn2_bits, float* d_thr_fast, uint32_t* d_canonical,
                          hipStream_t s);
// Every entry of every hit list of a completed row range (lists [nq][cap] {fast score bits, row}, min(counts[q], cap)
// entries each; max_count = the largest of them, known to the host): canonical score, comparison with the caller's
// threshold, running max |fast - canonical| into d_max_err (float bits), qualifying rows appended to the pool.
void launch_range_rescore_cut(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q, uint32_t nq,
                              const uint2* d_lists, const uint32_t* d_counts, uint32_t cap, uint32_t max_count, const float* d_thresholds,
                              const IdMap& idmap, const RangePool& pool, uint32_t* d_max_err, hipStream_t s);
// Canonical route: a block of canonical scores d_scores[i * score_ld + c], c < n, of n_queries queries -- query
// query_index[i] (host array, at most 8 entries) or, with query_index null, query q0 + i -- compared with the caller's
// thresholds and appended.  Column c is row d_list[c] (d_list non-null: the gather route's ascending row list) or row
// c itself, which is left out when set in d_row_mask (may be null).
void launch_range_cut_scores(const float* d_scores, uint64_t score_ld, uint64_t n, uint32_t n_queries, const uint32_t* query_index,
                             uint32_t q0, int metric, const float* d_thresholds, const uint32_t* d_row_mask, const uint32_t* d_list,
                             const IdMap& idmap, const RangePool& pool, hipStream_t s);
// Sort n pool entries ascending by (key, id): bitonic chunks in LDS, then merge passes between d_a and d_b.  Returns the
// buffer that holds the result (d_a or d_b).
RangeHit* launch_range_sort(RangeHit* d_a, RangeHit* d_b, uint64_t n, hipStream_t s);
// Sorted entries -> the caller's arrays: ids and canonical score bits.
void launch_range_emit(const RangeHit* d_sorted, uint64_t n, int metric, uint64_t* d_out_ids, float* d_out_scores, hipStream_t s);

}  // namespace vrod
