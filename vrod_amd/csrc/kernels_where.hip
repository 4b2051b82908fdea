// kernels_where.hip -- the device side of a search with a tags + value-interval predicate per query (vrod_search_where,
// gfx950): the rows of the corpus grouped by the predicates a batch asks for, and the effective row mask of one
// predicate for the groups that take a dense scan.
//
// The reference has no collections and no attributes (src/database/mod.rs:6-10, "//TODO collections"); a signed 64-bit
// value per row beside the tag mask is what lets one batch carry queries that each see their own time window, price
// range or version bound of one handle's rows.
//
// The kernels are those of kernels_tag.hip with a wider test: a lane holds its row's tags AND value, the wave walks the
// pass's predicate table in LDS (five words per group, every lane reads the same entry: a broadcast), a ballot per
// group gives the group's count in the wave and, below the lane, the row's rank in it.  One wave per block of rows, no
// atomic anywhere; pass 1 counts per (block, group), launch_group_prefix turns the counts into each block's first
// position within the group, pass 2 repeats the walk and writes the rows in ascending order.  Either array may be null
// (never set: every row carries 0), so a handle with only one of the two pays for one load per row.
#include "where_plan.h"
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

// SCATTER false: cnt[b * cnt_ld + g] = eligible matching rows of group g in block b.
// SCATTER true : cnt holds each block's first position within the group (launch_group_prefix), seg_off[g] the group's
//                first entry in `lists` (kNoSegment: the group wants no list); the rows are written in ascending order.
// tags == null / vals == null: every row carries 0.  mask (may be null): bit set = the row is not eligible.
template <bool SCATTER>
__global__ __launch_bounds__(64) void where_group_kernel(const uint64_t* __restrict__ tags, const int64_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ mask, uint64_t count, uint32_t rows_per_block,
                                                         const WherePred* __restrict__ table, uint32_t G, uint32_t* __restrict__ cnt,
                                                         uint32_t cnt_ld, const uint32_t* __restrict__ seg_off, uint32_t* __restrict__ lists) {
    extern __shared__ uint64_t lds64[];
    uint64_t* tab = lds64;                                // [G][5] any, all, none, lo, hi (the ends as their bits)
    uint32_t* ctr = (uint32_t*)(lds64 + 5 * (size_t)G);   // [G] running count / next position (kNoSegment: no list)
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < G; i += 64) {
        tab[5 * i] = table[i].any;
        tab[5 * i + 1] = table[i].all;
        tab[5 * i + 2] = table[i].none;
        tab[5 * i + 3] = (uint64_t)table[i].lo;
        tab[5 * i + 4] = (uint64_t)table[i].hi;
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
        const uint64_t t = ok && tags ? tags[r] : 0ull;
        const int64_t v = ok && vals ? vals[r] : 0ll;
        if (!__ballot(ok)) continue;
        for (uint32_t g = 0; g < G; ++g) {
            uint32_t c = 0;
            if constexpr (SCATTER) {
                c = ctr[g];   // the same word for every lane
                if (c == kNoSegment) continue;   // a wide group of the pass: no list, so no test either
            }
            const uint64_t* p = tab + 5 * (size_t)g;
            const bool hit = ok && where_matches(t, v, p[0], p[1], p[2], (int64_t)p[3], (int64_t)p[4]);
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
__global__ __launch_bounds__(256) void where_group_mask_kernel(const uint64_t* __restrict__ tags, const int64_t* __restrict__ vals,
                                                               const uint32_t* __restrict__ mask, uint64_t count, uint64_t n_words, WherePred p,
                                                               uint32_t* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool off = r >= count;
    if (!off && mask) off = (mask[r >> 5] >> (r & 31u)) & 1u;
    if (!off) off = !where_matches(tags ? tags[r] : 0ull, vals ? vals[r] : 0ll, p.any, p.all, p.none, p.lo, p.hi);
    const unsigned long long bits = __ballot(off);
    const uint32_t lane = threadIdx.x & 63u;
    if ((lane & 31u) == 0u && (r >> 5) < n_words) out[r >> 5] = (uint32_t)(lane ? bits >> 32 : bits);
}

// ------------------------------------------------------------------ launchers
static_assert(kWhereLdsPerGroup == sizeof(WherePred) + 4 && kWhereGroupsPerPass * kWhereLdsPerGroup <= 64 * 1024,
              "the pass's table fits the LDS of a plain launch");

void launch_where_group_count(const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block,
                              const WherePred* d_table, uint32_t G, uint32_t* d_cnt, uint32_t cnt_ld, hipStream_t s) {
    if (!G || !count) return;
    const uint32_t n_blocks = (uint32_t)((count + rows_per_block - 1) / rows_per_block);
    where_group_kernel<false><<<n_blocks, 64, (size_t)G * kWhereLdsPerGroup, s>>>(d_tags, d_vals, d_mask, count, rows_per_block, d_table, G, d_cnt,
                                                                                 cnt_ld, nullptr, nullptr);
}

void launch_where_group_scatter(const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block,
                                const WherePred* d_table, uint32_t G, const uint32_t* d_cnt, uint32_t cnt_ld, const uint32_t* d_seg_off,
                                uint32_t* d_lists, hipStream_t s) {
    if (!G || !count) return;
    const uint32_t n_blocks = (uint32_t)((count + rows_per_block - 1) / rows_per_block);
    where_group_kernel<true><<<n_blocks, 64, (size_t)G * kWhereLdsPerGroup, s>>>(d_tags, d_vals, d_mask, count, rows_per_block, d_table, G,
                                                                                const_cast<uint32_t*>(d_cnt), cnt_ld, d_seg_off, d_lists);
}

void launch_where_group_mask(const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_mask, uint64_t count, uint64_t n_words,
                             const WherePred& p, uint32_t* d_out, hipStream_t s) {
    if (!n_words) return;
    where_group_mask_kernel<<<(unsigned)((n_words * 32 + 255) / 256), 256, 0, s>>>(d_tags, d_vals, d_mask, count, n_words, p, d_out);
}

}  // namespace vrod
