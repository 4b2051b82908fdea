// kernels_group.hip -- the device side of a grouped search (vrod_search_grouped, gfx950): the best row of each label,
// the k best labels per query.
//
// A search's result list is sorted by (score, id), so the first entry of a list that carries a label is that label's
// best row among the list's rows.  group_dedupe_kernel keeps exactly those entries: one work-group per query puts the
// labels the query has taken so far and the labels of the list's entries into LDS, hashes them into a table whose slots
// hold the SMALLEST position that carries the slot's label (claimed by a compare-and-swap, lowered by an atomic
// minimum: no lock, no wait between lanes), and appends the entries that own their slot to the query's output in list
// order (ballot + popcount ranks, no atomics).  Labels taken earlier sit in front of the list's entries, so they own
// their slots and a list entry that repeats one is dropped.
//
// group_mask_kernel serves the dense stage (a few labels own more of a query's best rows than one list holds): per
// query the row mask "deleted, filtered out, or of a label already taken", as a bitmap the select chain reads in place
// of the handle's own.  A bitmap rather than a worst score written over the score: an eligible row's own score may be
// the worst there is (an IP score of -inf, a NaN), and a masked row must rank below that too -- it must be absent.
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "group_plan.h"

namespace vrod {

constexpr uint32_t kGroupEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t group_hash(uint32_t label, uint32_t shift) { return (label * 2654435761u) >> shift; }

// table[slot] = the smallest position i with lab[i] == the slot's label.  The table always keeps empty slots
// (group_plan.h), so every probe sequence ends.
__device__ __forceinline__ void group_insert(uint32_t* table, uint32_t slot_mask, uint32_t shift, const uint32_t* lab, uint32_t i) {
    const uint32_t label = lab[i];
    uint32_t h = group_hash(label, shift);
    for (;;) {
        const uint32_t old = atomicCAS(&table[h], kGroupEmpty, i);
        if (old == kGroupEmpty) return;
        if (lab[old] == label) { atomicMin(&table[h], i); return; }   // (a slot never changes its label)
        h = (h + 1) & slot_mask;
    }
}

__device__ __forceinline__ uint32_t group_find(const uint32_t* table, uint32_t slot_mask, uint32_t shift, const uint32_t* lab, uint32_t label) {
    uint32_t h = group_hash(label, shift);
    for (;;) {
        const uint32_t j = table[h];
        if (j == kGroupEmpty || lab[j] == label) return j;
        h = (h + 1) & slot_mask;
    }
}

// Block b: list b (cand_ids / cand_scores + b * k1: a search's result row, best first, unfilled slots last) of query
// qidx[b] (b itself without qidx).  found[q] < k results stand in the query's output row already, their labels in
// out_labels; the list's first entry of every label not among them is appended while the row has room.  found[q]
// becomes the new count, valid[q] the list's real entries.  labels == null: every row carries label 0.
__global__ __launch_bounds__(256) void group_dedupe_kernel(const uint64_t* __restrict__ cand_ids, const float* __restrict__ cand_scores,
                                                           uint32_t k1, const uint32_t* __restrict__ labels, uint64_t id_offset,
                                                           const uint32_t* __restrict__ qidx, uint32_t k, uint32_t slots, uint32_t shift,
                                                           uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                           uint32_t* __restrict__ out_labels, uint32_t* __restrict__ found,
                                                           uint32_t* __restrict__ valid) {
    extern __shared__ uint32_t lds[];
    uint32_t* table = lds;           // [slots]
    uint32_t* lab = lds + slots;     // [have + k1]: the labels taken so far, then the list's
    __shared__ uint32_t wave_cnt[4];
    __shared__ uint32_t n_valid;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = qidx ? qidx[blockIdx.x] : blockIdx.x;
    const uint64_t* ids = cand_ids + (uint64_t)blockIdx.x * k1;
    const float* sc = cand_scores + (uint64_t)blockIdx.x * k1;
    const uint64_t out0 = (uint64_t)q * k;
    const uint32_t have = found[q];
    if (have >= k) return;   // (a full row takes nothing more; the whole work-group leaves)
    for (uint32_t i = tid; i < slots; i += 256) table[i] = kGroupEmpty;
    for (uint32_t i = tid; i < have; i += 256) lab[i] = out_labels[out0 + i];
    if (tid == 0) n_valid = 0u;
    __syncthreads();
    uint32_t nv = 0;
    for (uint32_t i = tid; i < k1; i += 256) {
        const uint64_t id = ids[i];
        const bool real = id != UINT64_MAX;
        lab[have + i] = real && labels ? labels[id - id_offset] : 0u;
        nv += real;
    }
    if (nv) atomicAdd(&n_valid, nv);
    __syncthreads();
    for (uint32_t i = tid; i < have + k1; i += 256)
        if (i < have || ids[i - have] != UINT64_MAX) group_insert(table, slots - 1, shift, lab, i);
    __syncthreads();
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint32_t base = have;   // (the same in every thread)
    for (uint32_t c0 = 0; c0 < k1 && base < k; c0 += 256) {
        const uint32_t i = c0 + tid;
        uint64_t id = UINT64_MAX;
        bool keep = false;
        if (i < k1) {
            id = ids[i];
            keep = id != UINT64_MAX && group_find(table, slots - 1, shift, lab, lab[have + i]) == have + i;
        }
        const unsigned long long mine = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = (uint32_t)__builtin_popcountll(mine);
        __syncthreads();
        uint32_t pos = base + (uint32_t)__builtin_popcountll(mine & below);
        for (uint32_t w = 0; w < wave; ++w) pos += wave_cnt[w];
        if (keep && pos < k) {
            out_ids[out0 + pos] = id;
            out_scores[out0 + pos] = sc[i];
            out_labels[out0 + pos] = lab[have + i];
        }
        base += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();   // (wave_cnt is written again by the next step)
    }
    if (tid == 0) {
        found[q] = base < k ? base : k;
        valid[q] = n_valid;
    }
}

// Block (x, a): rows [x * kGroupMaskRowsPerBlock, ...) of the mask of query qidx[a], out + a * n_words.  Bit r set = row
// r is set in base_mask (may be null), lies at or beyond `count`, or carries one of the found[q] labels at
// out_labels[q * k ...].  A wave covers 256 rows per step: a lane reads the labels of 4 rows as one 16-byte word, the
// 8 lanes of a mask word fold their nibbles by xor shuffles.  `rows` = count rounded up to 256 (within the capacity the
// label array and the masks are allocated for).
__global__ __launch_bounds__(256) void group_mask_kernel(const uint32_t* __restrict__ labels, const uint32_t* __restrict__ base_mask,
                                                         uint64_t count, uint64_t rows, uint64_t n_words, const uint32_t* __restrict__ qidx,
                                                         const uint32_t* __restrict__ out_labels, const uint32_t* __restrict__ found,
                                                         uint32_t k, uint32_t slots, uint32_t shift, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t lds[];
    uint32_t* table = lds;           // [slots]
    uint32_t* taken = lds + slots;   // [have]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = qidx[blockIdx.y];
    const uint32_t have = found[q];
    for (uint32_t i = tid; i < slots; i += 256) table[i] = kGroupEmpty;
    for (uint32_t i = tid; i < have; i += 256) taken[i] = out_labels[(uint64_t)q * k + i];
    __syncthreads();
    for (uint32_t i = tid; i < have; i += 256) group_insert(table, slots - 1, shift, taken, i);
    __syncthreads();
    uint32_t* o = out + (uint64_t)blockIdx.y * n_words;
    const uint64_t begin = (uint64_t)blockIdx.x * kGroupMaskRowsPerBlock;
    const uint64_t end = begin + kGroupMaskRowsPerBlock < rows ? begin + kGroupMaskRowsPerBlock : rows;
    for (uint64_t r0 = begin + (uint64_t)wave * 256; r0 < end; r0 += 1024) {
        const uint64_t r = r0 + 4ull * lane;
        u32x4_t l4 = {0u, 0u, 0u, 0u};
        if (labels && have) l4 = *(const u32x4_t*)(labels + r);
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bool off = r + e >= count;
            if (!off && have) off = group_find(table, slots - 1, shift, taken, l4[e]) != kGroupEmpty;
            v |= (uint32_t)off << e;
        }
        v <<= 4u * (lane & 7u);
        v |= __shfl_xor(v, 1);
        v |= __shfl_xor(v, 2);
        v |= __shfl_xor(v, 4);
        const uint64_t word = (r0 >> 5) + (lane >> 3);
        if ((lane & 7u) == 0u) o[word] = base_mask ? v | base_mask[word] : v;
    }
}

// ------------------------------------------------------------------ launchers
static uint32_t hash_shift(uint32_t slots) {
    uint32_t bits = 0;
    while ((1u << bits) < slots) ++bits;
    return 32 - bits;
}

void launch_group_dedupe(const uint64_t* d_cand_ids, const float* d_cand_scores, uint32_t k1, uint32_t n_lists, const uint32_t* d_labels,
                         uint64_t id_offset, const uint32_t* d_qidx, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                         uint32_t* d_out_labels, uint32_t* d_found, uint32_t* d_valid, hipStream_t s) {
    if (!n_lists) return;
    const uint32_t slots = group_dedupe_slots(k, k1);
    const size_t lds = ((size_t)slots + group_dedupe_entries(k, k1)) * 4;
    group_dedupe_kernel<<<n_lists, 256, lds, s>>>(d_cand_ids, d_cand_scores, k1, d_labels, id_offset, d_qidx, k, slots, hash_shift(slots),
                                                  d_out_ids, d_out_scores, d_out_labels, d_found, d_valid);
}

void launch_group_mask(const uint32_t* d_labels, const uint32_t* d_base_mask, uint64_t count, uint64_t n_words, const uint32_t* d_qidx,
                       uint32_t n_queries, const uint32_t* d_out_labels, const uint32_t* d_found, uint32_t k, uint32_t* d_out, hipStream_t s) {
    if (!n_queries || !count) return;
    const uint64_t rows = (count + 255) / 256 * 256;
    const uint32_t slots = group_dedupe_slots(k, 0);
    const size_t lds = ((size_t)slots + k) * 4;
    const dim3 grid((unsigned)((rows + kGroupMaskRowsPerBlock - 1) / kGroupMaskRowsPerBlock), n_queries);
    group_mask_kernel<<<grid, 256, lds, s>>>(d_labels, d_base_mask, count, rows, n_words, d_qidx, d_out_labels, d_found, k, slots,
                                             hash_shift(slots), d_out);
}

}  // namespace vrod
