// kernels_label.hip -- row labels (vrod_index_set_labels) and the device side of a labelled search
// (vrod_search_labeled, gfx950): the rows of the corpus grouped by the labels a batch asks for, in ONE pass over the
// label array, and the effective row mask of one label for the groups that take a dense scan.
//
// The reference has no collections (src/database/mod.rs:6-10, "//TODO collections"); a label per row is what lets one
// handle hold many tenants' rows and one batch carry many tenants' queries.
//
// Grouping is a counting sort that keeps row order: block b owns rows [b * R, (b + 1) * R) and walks them 64 at a time
// with ONE wave.  A lane finds its row's group by a binary search of the batch's sorted labels in LDS; the wave then
// peels off the groups present in it one by one -- the lowest lane still waiting names the group, a ballot finds the
// lanes that share it, a popcount below the lane is the row's rank -- so that rows of one group leave the wave in lane
// (= row) order with no atomic anywhere.  Pass 1 counts per (block, group), the prefix pass turns the counts into each
// block's first position within the group, pass 2 repeats the walk and writes the rows.  The ascending order within a
// group is what makes the score columns' tie-break the tie-break by id.
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

// The first steps of the search read one word for all lanes (a broadcast), the last ones neighbouring words: the
// table costs LDS bank conflicts only in between, and 12 steps at the most.
__device__ __forceinline__ uint32_t find_group(const uint32_t* tab, uint32_t G, uint32_t label) {
    uint32_t lo = 0, hi = G;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid] < label) lo = mid + 1; else hi = mid;
    }
    return lo < G && tab[lo] == label ? lo : kNoSegment;
}

// SCATTER false: cnt[b * cnt_ld + g] = eligible rows of group g in block b.
// SCATTER true : cnt holds each block's first position within the group (launch_group_prefix), seg_off[g] the group's
//                first entry in `lists` (kNoSegment: the group wants no list); the rows are written in ascending order.
// labels == null: every row carries label 0.  mask (may be null): bit set = the row is not eligible.
template <bool SCATTER>
__global__ __launch_bounds__(64) void label_group_kernel(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ mask,
                                                         uint64_t count, uint32_t rows_per_block, const uint32_t* __restrict__ table,
                                                         uint32_t G, uint32_t* __restrict__ cnt, uint32_t cnt_ld,
                                                         const uint32_t* __restrict__ seg_off, uint32_t* __restrict__ lists) {
    extern __shared__ uint32_t lds[];
    uint32_t* tab = lds;        // [G] sorted labels
    uint32_t* ctr = lds + G;    // [G] running count / next position (kNoSegment: no list)
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
        uint32_t g = kNoSegment;
        if (ok) g = find_group(tab, G, labels ? labels[r] : 0u);
        unsigned long long todo = __ballot(g != kNoSegment);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const uint32_t gl = (uint32_t)__builtin_amdgcn_readlane((int)g, leader);
            const unsigned long long same = __ballot(g == gl);
            const uint32_t c = ctr[gl];
            if constexpr (SCATTER) {
                if (g == gl && c != kNoSegment) lists[c + (uint32_t)__builtin_popcountll(same & below)] = (uint32_t)r;
            }
            __builtin_amdgcn_wave_barrier();   // every lane has read ctr[gl] before the leader moves it on
            if ((int)lane == leader && c != kNoSegment) ctr[gl] = c + (uint32_t)__builtin_popcountll(same);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            todo &= ~same;
        }
    }
    if constexpr (!SCATTER) {
        __syncthreads();
        for (uint32_t i = lane; i < G; i += 64) cnt[(uint64_t)blockIdx.x * cnt_ld + i] = ctr[i];
    }
}

// cnt [n_blocks][G] -> exclusive prefix over the blocks, per group; total[g] = the group's eligible rows.
// Thread (x, y) of a 64 x 16 block: group 64 * blockIdx.x + x, the y-th sixteenth of the blocks.
__global__ __launch_bounds__(1024) void label_prefix_kernel(uint32_t* __restrict__ cnt, uint32_t n_blocks, uint32_t G,
                                                            uint32_t* __restrict__ total) {
    __shared__ uint32_t part[16][64];
    const uint32_t x = threadIdx.x, y = threadIdx.y, g = blockIdx.x * 64 + x;
    const uint32_t per = (n_blocks + 15) / 16;
    const uint32_t b0 = y * per < n_blocks ? y * per : n_blocks, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    uint32_t sum = 0;
    if (g < G)
        for (uint32_t b = b0; b < b1; ++b) sum += cnt[(uint64_t)b * G + g];
    part[y][x] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t i = 0; i < y; ++i) run += part[i][x];
    if (g < G) {
        for (uint32_t b = b0; b < b1; ++b) {
            const uint32_t c = cnt[(uint64_t)b * G + g];
            cnt[(uint64_t)b * G + g] = run;
            run += c;
        }
        if (y == 15) total[g] = run;
    }
}

// The effective mask of one label, for a dense scan: bit r set = row r is masked by `mask` (may be null), carries
// another label, or lies at or beyond `count`.  A wave covers 64 rows; lanes 0 and 32 write the ballot's two words.
__global__ __launch_bounds__(256) void label_group_mask_kernel(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ mask,
                                                               uint64_t count, uint64_t n_words, uint32_t label, uint32_t* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool off = r >= count;
    if (!off && mask) off = (mask[r >> 5] >> (r & 31u)) & 1u;
    if (!off) off = (labels ? labels[r] : 0u) != label;
    const unsigned long long bits = __ballot(off);
    const uint32_t lane = threadIdx.x & 63u;
    if ((lane & 31u) == 0u && (r >> 5) < n_words) out[r >> 5] = (uint32_t)(lane ? bits >> 32 : bits);
}

// dst row i = src row idx[i], rows of `dim` floats (the raw queries of one label's group)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t dim,
                                                          float* __restrict__ dst) {
    const float* row = src + (uint64_t)idx[blockIdx.x] * dim;
    for (uint32_t j = threadIdx.x; j < dim; j += 256) dst[(uint64_t)blockIdx.x * dim + j] = row[j];
}

// ------------------------------------------------------------------ launchers
void launch_label_group_count(const uint32_t* d_labels, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block,
                              const uint32_t* d_table, uint32_t G, uint32_t* d_cnt, uint32_t cnt_ld, hipStream_t s) {
    if (!G || !count) return;
    const uint32_t n_blocks = (uint32_t)((count + rows_per_block - 1) / rows_per_block);
    label_group_kernel<false><<<n_blocks, 64, (size_t)G * 8, s>>>(d_labels, d_mask, count, rows_per_block, d_table, G, d_cnt, cnt_ld, nullptr,
                                                                  nullptr);
}

void launch_group_prefix(uint32_t* d_cnt, uint32_t n_blocks, uint32_t G, uint32_t* d_total, hipStream_t s) {
    if (!G || !n_blocks) return;
    label_prefix_kernel<<<(G + 63) / 64, dim3(64, 16), 0, s>>>(d_cnt, n_blocks, G, d_total);
}

void launch_label_group_scatter(const uint32_t* d_labels, const uint32_t* d_mask, uint64_t count, uint32_t rows_per_block,
                                const uint32_t* d_table, uint32_t G, const uint32_t* d_cnt, uint32_t cnt_ld, const uint32_t* d_seg_off,
                                uint32_t* d_lists, hipStream_t s) {
    if (!G || !count) return;
    const uint32_t n_blocks = (uint32_t)((count + rows_per_block - 1) / rows_per_block);
    label_group_kernel<true><<<n_blocks, 64, (size_t)G * 8, s>>>(d_labels, d_mask, count, rows_per_block, d_table, G, const_cast<uint32_t*>(d_cnt),
                                                                 cnt_ld, d_seg_off, d_lists);
}

void launch_label_group_mask(const uint32_t* d_labels, const uint32_t* d_mask, uint64_t count, uint64_t n_words, uint32_t label,
                             uint32_t* d_out, hipStream_t s) {
    if (!n_words) return;
    label_group_mask_kernel<<<(unsigned)((n_words * 32 + 255) / 256), 256, 0, s>>>(d_labels, d_mask, count, n_words, label, d_out);
}

void launch_gather_rows(const float* d_src, const uint32_t* d_idx, uint32_t n, uint32_t dim, float* d_dst, hipStream_t s) {
    if (!n) return;
    gather_rows_kernel<<<n, 256, 0, s>>>(d_src, d_idx, dim, d_dst);
}

}  // namespace vrod
