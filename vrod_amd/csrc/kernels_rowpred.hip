// kernels_rowpred.hip -- the device side of the row-predicate operations (vrod_index_count_where, _select_where,
// _delete_where, _set_filter_where, _set_tags_where; gfx950): a predicate over a row's tags, value and label evaluated
// on the rows themselves, at the speed the three columns can be read.
//
// The reference has no collections and no attributes (src/database/mod.rs:6-10, "//TODO collections"); its DELETE names
// one row.  Expiry, the removal of a document and a where-clause on every search form need the predicate as an
// operation of its own.
//
// Three passes, all cut the same way: work-group b owns rows [b * R, (b + 1) * R), R = kRowPredRowsPerGroup, and a wave
// covers 64 rows at a time -- a lane loads its row's tags, value and label (a column that does not exist costs no
// load), a ballot gives the two 32-bit hit words and their popcount.
//   count  : the counting walk of kernels_pred.hip over the three columns (launch_pred_group_count with RowPredRows
//            and R rows a block), launch_group_prefix sums its per-(group, predicate) counts;
//   hits   : one predicate; the hit bitmap and the group's count.  The bitmap is all that crosses to the host for a
//            delete, a filter or a retag; RETAG also rewrites the tags of the rows it marks, in the same pass;
//   scatter: a wave reads its group's 64 hit words back, a lane a word, and writes the ids in ascending order from the
//            group's first position (the prefix of the counts).
// No atomic anywhere: counts and order do not depend on how the groups are scheduled.
#include "rowpred_plan.h"
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

// hits: bit r set = row r is in scope and matches p (RETAG: and its tags change under (t & ~clear_bits) | set_bits,
// which is then what the row carries).  Written for the rows below count rounded up to 64: row_pred_hit_words(count)
// words.  cnt (may be null): cnt[b] = the bits group b set.
template <bool RETAG>
__global__ __launch_bounds__(kRowPredThreads) void rowpred_hits_kernel(uint64_t* __restrict__ tags, const int64_t* __restrict__ vals,
                                                                       const uint32_t* __restrict__ labels,
                                                                       const uint32_t* __restrict__ scope, uint64_t count, RowPred p,
                                                                       uint64_t set_bits, uint64_t clear_bits, uint32_t* __restrict__ hits,
                                                                       uint32_t* __restrict__ cnt) {
    __shared__ uint32_t part[kRowPredThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t begin = (uint64_t)blockIdx.x * kRowPredRowsPerGroup;
    uint32_t n = 0;
    for (uint32_t i = 0; i < kRowPredRowsPerGroup; i += kRowPredThreads) {
        const uint64_t r0 = begin + i + wave * 64;   // the wave's 64 rows: uniform
        if (r0 >= count) break;
        const uint64_t r = r0 + lane;
        const bool ok = row_in_scope(scope, r, count);
        const uint64_t t = ok && tags ? tags[r] : 0ull;
        const int64_t v = ok && vals ? vals[r] : 0ll;
        const uint32_t l = ok && labels ? labels[r] : 0u;
        bool hit = ok && row_pred_matches(t, v, l, p);
        if constexpr (RETAG) {
            const uint64_t t1 = (t & ~clear_bits) | set_bits;
            hit = hit && t1 != t;
            if (hit) tags[r] = t1;
        }
        const unsigned long long bits = __ballot(hit);
        if ((lane & 31u) == 0u) hits[r >> 5] = (uint32_t)(lane ? bits >> 32 : bits);
        n += (uint32_t)__builtin_popcountll(bits);
    }
    if (!cnt) return;
    if (lane == 0) part[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kRowPredThreads / 64; ++w) sum += part[w];
        cnt[blockIdx.x] = sum;
    }
}

// out[first[b] + j] = id_offset + the j-th set bit of group b's 64 hit words: the whole selection ascending.
__global__ __launch_bounds__(64) void rowpred_scatter_kernel(const uint32_t* __restrict__ hits, uint64_t n_words,
                                                             const uint32_t* __restrict__ first, uint64_t id_offset,
                                                             uint64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint64_t w = (uint64_t)blockIdx.x * (kRowPredRowsPerGroup / 32) + lane;
    uint32_t word = w < n_words ? hits[w] : 0u;
    const uint32_t mine = (uint32_t)__builtin_popcount(word);
    uint32_t upto = mine;   // inclusive prefix over the lanes
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(upto, d);
        if (lane >= d) upto += o;
    }
    uint64_t at = (uint64_t)first[blockIdx.x] + (upto - mine);
    while (word) {
        out[at++] = id_offset + w * 32 + (uint32_t)__builtin_ctz(word);
        word &= word - 1u;
    }
}

// ------------------------------------------------------------------ launchers
void launch_rowpred_hits(const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope, uint64_t count,
                         const RowPred& p, uint32_t* d_hits, uint32_t* d_cnt, hipStream_t s) {
    if (!count) return;
    rowpred_hits_kernel<false><<<row_pred_groups(count), kRowPredThreads, 0, s>>>(const_cast<uint64_t*>(d_tags), d_vals, d_labels, d_scope, count,
                                                                                 p, 0ull, 0ull, d_hits, d_cnt);
}

void launch_rowpred_retag(uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope, uint64_t count,
                          const RowPred& p, uint64_t set_bits, uint64_t clear_bits, uint32_t* d_hits, hipStream_t s) {
    if (!count) return;
    rowpred_hits_kernel<true><<<row_pred_groups(count), kRowPredThreads, 0, s>>>(d_tags, d_vals, d_labels, d_scope, count, p, set_bits, clear_bits,
                                                                                d_hits, nullptr);
}

void launch_rowpred_scatter(const uint32_t* d_hits, uint64_t count, const uint32_t* d_first, uint64_t id_offset, uint64_t* d_out, hipStream_t s) {
    if (!count) return;
    rowpred_scatter_kernel<<<row_pred_groups(count), 64, 0, s>>>(d_hits, row_pred_hit_words(count), d_first, id_offset, d_out);
}

}  // namespace vrod
