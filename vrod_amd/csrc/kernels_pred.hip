// kernels_pred.hip -- the device side of every operation that evaluates a batch's predicates on the rows' side columns
// (vrod_search_tagged, vrod_search_where, vrod_index_count_where; gfx950): the rows of the corpus grouped by the
// predicates a batch asks for, and the effective row mask of one predicate for the groups that take a dense scan.
//
// The reference has no collections and no attributes (src/database/mod.rs:6-10, "//TODO collections"); a 64-bit tag
// mask, a signed 64-bit value and a label per row, and a predicate over them per query, are what let one batch carry
// queries that each see their own attribute subset, time window or tenant of one handle's rows.
//
// Grouping follows kernels_label.hip -- a counting sort that keeps row order, block b owning rows [b * R, (b + 1) * R)
// and walking them 64 at a time with ONE wave, no atomic anywhere -- with one difference: a row belongs to every group
// whose predicate it matches, not to one.  So there is nothing to search for: a lane holds its row's columns (a column
// that was never set is null, every row carries 0 and the lane pays no load for it), the wave walks the pass's
// predicate table in LDS (every lane reads the same entry: a broadcast), and for each group a ballot of the matching
// lanes gives the group's count in the wave and, below the lane, the row's rank in it.  Pass 1 counts per (block,
// group), launch_group_prefix turns the counts into each block's first position within the group, pass 2 repeats the
// walk and writes the rows.  The ascending order within a group is what makes the score columns' tie-break the
// tie-break by id.  The test costs O(groups) per row where a label costs O(log groups).
//
// One walk for three kinds of row (vrod_kernels.h TagRows, WhereRows, RowPredRows): what a lane loads, and the test,
// which is the function the host shares (tag_plan.h, where_plan.h, rowpred_plan.h).
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

struct TagRow { uint64_t t; };
struct WhereRow { uint64_t t; int64_t v; };
struct LabelledRow { uint64_t t; int64_t v; uint32_t l; };
// ok false: the row is out of range or not eligible, nothing is read
__device__ __forceinline__ TagRow load_row(const TagRows& c, uint64_t r, bool ok) { return {ok && c.tags ? c.tags[r] : 0ull}; }
__device__ __forceinline__ WhereRow load_row(const WhereRows& c, uint64_t r, bool ok) {
    return {ok && c.tags ? c.tags[r] : 0ull, ok && c.vals ? c.vals[r] : 0ll};
}
__device__ __forceinline__ LabelledRow load_row(const RowPredRows& c, uint64_t r, bool ok) {
    return {ok && c.tags ? c.tags[r] : 0ull, ok && c.vals ? c.vals[r] : 0ll, ok && c.labels ? c.labels[r] : 0u};
}
__device__ __forceinline__ bool row_matches(const TagRow& w, const TagPred& p) { return tag_matches(w.t, p.any, p.all, p.none); }
__device__ __forceinline__ bool row_matches(const WhereRow& w, const WherePred& p) {
    return where_matches(w.t, w.v, p.any, p.all, p.none, p.lo, p.hi);
}
__device__ __forceinline__ bool row_matches(const LabelledRow& w, const RowPred& p) { return row_pred_matches(w.t, w.v, w.l, p); }

// SCATTER false: cnt[b * cnt_ld + g] = eligible matching rows of group g in block b.
// SCATTER true : cnt holds each block's first position within the group (launch_group_prefix), seg_off[g] the group's
//                first entry in `lists` (kNoSegment: the group wants no list); the rows are written in ascending order.
// mask (may be null): bit set = the row is not eligible.
template <typename Rows, bool SCATTER>
__global__ __launch_bounds__(64) void pred_group_kernel(Rows rows, const uint32_t* __restrict__ mask, uint64_t count, uint32_t rows_per_block,
                                                        const typename Rows::Pred* __restrict__ table, uint32_t G, uint32_t* __restrict__ cnt,
                                                        uint32_t cnt_ld, const uint32_t* __restrict__ seg_off, uint32_t* __restrict__ lists) {
    using Pred = typename Rows::Pred;
    extern __shared__ uint64_t lds64[];
    Pred* tab = (Pred*)lds64;              // [G]
    uint32_t* ctr = (uint32_t*)(tab + G);   // [G] running count / next position (kNoSegment: no list)
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < G; i += 64) {
        tab[i] = table[i];
        if constexpr (SCATTER) ctr[i] = seg_off[i] == kNoSegment ? kNoSegment : seg_off[i] + cnt[(uint64_t)blockIdx.x * cnt_ld + i];
        else ctr[i] = 0u;
    }
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * rows_per_block;
    const uint64_t end = begin + rows_per_block < count ? begin + rows_per_block : count;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (uint64_t r0 = begin; r0 < end; r0 += 64) {
        const uint64_t r = r0 + lane;
        bool ok = r < end;
        if (ok && mask) ok = !((mask[r >> 5] >> (r & 31u)) & 1u);
        const auto row = load_row(rows, r, ok);
        if (!__ballot(ok)) continue;
        for (uint32_t g = 0; g < G; ++g) {
            uint32_t c = 0;
            if constexpr (SCATTER) {
                c = ctr[g];   // the same word for every lane
                if (c == kNoSegment) continue;   // a wide group of the pass: no list, so no test either
            }
            const bool hit = ok && row_matches(row, tab[g]);
            const unsigned long long hits = __ballot(hit);
            if (!hits) continue;
            if constexpr (SCATTER) {
                if (hit) lists[c + (uint32_t)__builtin_popcountll(hits & below)] = (uint32_t)r;
                __builtin_amdgcn_wave_barrier();   // every lane has read ctr[g] before lane 0 moves it on
                if (lane == 0) ctr[g] = c + (uint32_t)__builtin_popcountll(hits);
            } else {
                if (lane == 0) ctr[g] += (uint32_t)__builtin_popcountll(hits);   // (only lane 0 ever touches it)
            }
        }
        // lane 0's counters are what every lane reads in the next 64 rows
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (!SCATTER) {
        __syncthreads();
        for (uint32_t i = lane; i < G; i += 64) cnt[(uint64_t)blockIdx.x * cnt_ld + i] = ctr[i];
    }
}

// The effective mask of one predicate, for a dense scan: bit r set = row r is masked by `mask` (may be null), does not
// match, or lies at or beyond `count`.  A wave covers 64 rows; lanes 0 and 32 write the ballot's two words.
template <typename Rows>
__global__ __launch_bounds__(256) void pred_group_mask_kernel(Rows rows, const uint32_t* __restrict__ mask, uint64_t count, uint64_t n_words,
                                                              typename Rows::Pred p, uint32_t* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool off = r >= count;
    if (!off && mask) off = (mask[r >> 5] >> (r & 31u)) & 1u;
    if (!off) off = !row_matches(load_row(rows, r, true), p);
    const unsigned long long bits = __ballot(off);
    const uint32_t lane = threadIdx.x & 63u;
    if ((lane & 31u) == 0u && (r >> 5) < n_words) out[r >> 5] = (uint32_t)(lane ? bits >> 32 : bits);
}

// ------------------------------------------------------------------ launchers
// A group's bytes of LDS: its predicate and its counter.
template <typename Pred> constexpr size_t kPredLds = sizeof(Pred) + 4;
static_assert(kTagLdsPerGroup == kPredLds<TagPred> && kTagGroupsPerPass * kTagLdsPerGroup <= 64 * 1024 &&
              kWhereLdsPerGroup == kPredLds<WherePred> && kWhereGroupsPerPass * kWhereLdsPerGroup <= 64 * 1024 &&
              sizeof(RowPred) == 48 && kRowPredLdsPerPred == kPredLds<RowPred> && kRowPredsPerPass * kRowPredLdsPerPred <= 64 * 1024,
              "the pass's table fits the LDS of a plain launch");

template <typename Rows>
void launch_pred_group_count(Rows rows, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block, const typename Rows::Pred* d_table,
                             uint32_t G, uint32_t* d_cnt, uint32_t cnt_ld, hipStream_t s) {
    if (!G || !count) return;
    const uint32_t n_blocks = (uint32_t)((count + rows_per_block - 1) / rows_per_block);
    pred_group_kernel<Rows, false><<<n_blocks, 64, G * kPredLds<typename Rows::Pred>, s>>>(rows, d_mask, count, rows_per_block, d_table, G, d_cnt,
                                                                                          cnt_ld, nullptr, nullptr);
}

template <typename Rows>
void launch_pred_group_scatter(Rows rows, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block, const typename Rows::Pred* d_table,
                               uint32_t G, const uint32_t* d_cnt, uint32_t cnt_ld, const uint32_t* d_seg_off, uint32_t* d_lists, hipStream_t s) {
    if (!G || !count) return;
    const uint32_t n_blocks = (uint32_t)((count + rows_per_block - 1) / rows_per_block);
    pred_group_kernel<Rows, true><<<n_blocks, 64, G * kPredLds<typename Rows::Pred>, s>>>(rows, d_mask, count, rows_per_block, d_table, G,
                                                                                         const_cast<uint32_t*>(d_cnt), cnt_ld, d_seg_off, d_lists);
}

template <typename Rows>
void launch_pred_group_mask(Rows rows, const uint32_t* d_mask, uint64_t count, uint64_t n_words, const typename Rows::Pred& p, uint32_t* d_out,
                            hipStream_t s) {
    if (!n_words) return;
    pred_group_mask_kernel<Rows><<<(unsigned)((n_words * 32 + 255) / 256), 256, 0, s>>>(rows, d_mask, count, n_words, p, d_out);
}

// tags and where: the three launches of a search; tags, value and label: the count of vrod_index_count_where
template void launch_pred_group_count(TagRows, const uint32_t*, uint64_t, uint32_t, const TagPred*, uint32_t, uint32_t*, uint32_t, hipStream_t);
template void launch_pred_group_count(WhereRows, const uint32_t*, uint64_t, uint32_t, const WherePred*, uint32_t, uint32_t*, uint32_t, hipStream_t);
template void launch_pred_group_count(RowPredRows, const uint32_t*, uint64_t, uint32_t, const RowPred*, uint32_t, uint32_t*, uint32_t, hipStream_t);
template void launch_pred_group_scatter(TagRows, const uint32_t*, uint64_t, uint32_t, const TagPred*, uint32_t, const uint32_t*, uint32_t,
                                        const uint32_t*, uint32_t*, hipStream_t);
template void launch_pred_group_scatter(WhereRows, const uint32_t*, uint64_t, uint32_t, const WherePred*, uint32_t, const uint32_t*, uint32_t,
                                        const uint32_t*, uint32_t*, hipStream_t);
template void launch_pred_group_mask(TagRows, const uint32_t*, uint64_t, uint64_t, const TagPred&, uint32_t*, hipStream_t);
template void launch_pred_group_mask(WhereRows, const uint32_t*, uint64_t, uint64_t, const WherePred&, uint32_t*, hipStream_t);

}  // namespace vrod
