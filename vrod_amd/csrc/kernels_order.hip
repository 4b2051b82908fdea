// kernels_order.hip -- the device side of ordered selection (vrod_index_select_ordered; gfx950): the top `limit` rows by
// (value, id) under a row predicate and after a keyset cursor, exact and deterministic.
//
// The reference keeps no attribute beside a row and orders nothing but scores (src/database/mod.rs); "the 100 newest
// rows of tenant L" needs a selection by a stored value.
//
// Four steps over the geometry of kernels_rowpred.hip (work-group b owns rows [b * R, (b + 1) * R), R =
// kRowPredRowsPerGroup, a wave covers 64 rows at a time), all in (key, id) space (order_plan.h):
//   hits    : rowpred_hits_kernel with the cursor test beside the predicate: the hit bitmap and each group's count;
//   select  : MSB-first radix select, 8 bits a round, for the key of rank `limit` among the hit rows.  A round's kernel
//             builds a histogram per work-group in LDS and adds it to the round's 256 bins; a one-wave kernel picks the
//             bucket (order_pick) and extends the prefix.  State stays on the device: no round trip between rounds;
//   collect : every hit row below the pivot key, and the pivot's tie class in ascending id up to the remainder, as
//             (key, id) records.  Positions come from per-group counts and a prefix over them;
//   sort    : bitonic over the at most 65536 records -- in LDS up to kOrderSortTile, above that the long-distance steps
//             in global memory -- then ids, and values recovered from the keys, to the outputs.
// Atomics only count (integer sums do not depend on their order); none decides a position or which tied row is kept.
#include "order_plan.h"
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

// A wave's 64 rows from r0 (a multiple of 64, below count): is this lane's row a hit?
__device__ __forceinline__ bool order_hit_bit(const uint32_t* __restrict__ hits, uint64_t r0, uint32_t lane) {
    return (hits[(r0 >> 5) + (lane >> 5)] >> (lane & 31u)) & 1u;
}

// hits: bit r set = row r is in scope, matches p and lies strictly after the cursor (has_cursor) in the call's order.
// Written for the rows below count rounded up to 64; cnt[b] = the bits group b set.
__global__ __launch_bounds__(kOrderThreads) void order_hits_kernel(const uint64_t* __restrict__ tags, const int64_t* __restrict__ vals,
                                                                   const uint32_t* __restrict__ labels, const uint32_t* __restrict__ scope,
                                                                   uint64_t count, RowPred p, bool desc, bool has_cursor, uint64_t ckey,
                                                                   uint64_t cid, uint64_t id_offset, uint32_t* __restrict__ hits,
                                                                   uint32_t* __restrict__ cnt) {
    __shared__ uint32_t part[kOrderThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t begin = (uint64_t)blockIdx.x * kRowPredRowsPerGroup;
    uint32_t n = 0;
    for (uint32_t i = 0; i < kRowPredRowsPerGroup; i += kOrderThreads) {
        const uint64_t r0 = begin + i + wave * 64;   // the wave's 64 rows: uniform
        if (r0 >= count) break;
        const uint64_t r = r0 + lane;
        const bool ok = row_in_scope(scope, r, count);
        const uint64_t t = ok && tags ? tags[r] : 0ull;
        const int64_t v = ok && vals ? vals[r] : 0ll;
        const uint32_t l = ok && labels ? labels[r] : 0u;
        bool hit = ok && row_pred_matches(t, v, l, p);
        if (has_cursor) hit = hit && order_after(order_key(v, desc), id_offset + r, ckey, cid);
        const unsigned long long bits = __ballot(hit);
        if ((lane & 31u) == 0u) hits[r >> 5] = (uint32_t)(lane ? bits >> 32 : bits);
        n += (uint32_t)__builtin_popcountll(bits);
    }
    if (lane == 0) part[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kOrderThreads / 64; ++w) sum += part[w];
        cnt[blockIdx.x] = sum;
    }
}

// The select's start: every round's bins zero, the prefix empty, the rank wanted = limit.
__global__ __launch_bounds__(kOrderBins) void order_begin_kernel(uint32_t* __restrict__ hist, OrderState* __restrict__ st, uint32_t limit) {
    for (uint32_t i = threadIdx.x; i < kOrderRounds * kOrderBins; i += kOrderBins) hist[i] = 0u;
    if (threadIdx.x == 0) *st = OrderState{0ull, limit};
}

// Round `round`: hist[d] += the group's hit rows whose higher digits equal the prefix chosen so far and whose digit is d.
__global__ __launch_bounds__(kOrderThreads) void order_hist_kernel(const uint32_t* __restrict__ hits, const int64_t* __restrict__ vals,
                                                                   uint64_t count, bool desc, uint32_t round,
                                                                   const OrderState* __restrict__ st, uint32_t* __restrict__ hist) {
    __shared__ uint32_t bins[kOrderBins];
    static_assert(kOrderThreads == kOrderBins, "a thread a bin");
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t begin = (uint64_t)blockIdx.x * kRowPredRowsPerGroup;
    const uint64_t prefix = st->pivot;
    for (uint32_t i = 0; i < kRowPredRowsPerGroup; i += kOrderThreads) {
        const uint64_t r0 = begin + i + wave * 64;
        if (r0 >= count) break;
        if (!order_hit_bit(hits, r0, lane)) continue;
        const uint64_t key = order_key(vals ? vals[r0 + lane] : 0ll, desc);
        if (order_in_prefix(key, prefix, round)) atomicAdd(&bins[order_digit(key, round)], 1u);
    }
    __syncthreads();
    const uint32_t mine = bins[threadIdx.x];
    if (mine) atomicAdd(&hist[threadIdx.x], mine);
}

// One wave: the bucket of the round's histogram that holds the wanted rank becomes the prefix's next digit.
__global__ __launch_bounds__(64) void order_pick_kernel(const uint32_t* __restrict__ hist, uint32_t round, OrderState* __restrict__ st) {
    __shared__ uint32_t bins[kOrderBins];
    for (uint32_t i = threadIdx.x; i < kOrderBins; i += 64) bins[i] = hist[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        const OrderPick pk = order_pick(bins, st->remaining);
        st->pivot |= (uint64_t)pk.digit << (56u - 8u * round);
        st->remaining = pk.remaining;
    }
}

// The rows a call takes, group by group.  A hit row is LOW when its key is below the pivot (take_all: always) and TIED
// when it equals the pivot.
//   WRITE == false: cnt2[b] = {low rows, tied rows} of group b.
//   WRITE == true : first[b * stride] is the group's first low position; with stride 2, first[b * 2 + 1] is the rank of
//                   its first tied row among all tied rows, ascending by id, and first[2 * groups] the low rows of the
//                   whole call.  Low rows go to their positions, tied rows of rank below st->remaining behind all low rows:
//                   n_rec records in all (a position at or past n_rec would be a bug of the select, and is not written).
template <bool WRITE>
__global__ __launch_bounds__(kOrderThreads) void order_collect_kernel(const uint32_t* __restrict__ hits, const int64_t* __restrict__ vals,
                                                                      uint64_t count, bool desc, uint64_t id_offset, bool take_all,
                                                                      const OrderState* __restrict__ st, uint32_t* __restrict__ cnt2,
                                                                      const uint32_t* __restrict__ first, uint32_t stride,
                                                                      uint32_t n_groups, uint64_t* __restrict__ rec, uint32_t n_rec) {
    constexpr uint32_t kIters = kRowPredRowsPerGroup / kOrderThreads, kWaves = kOrderThreads / 64;
    __shared__ uint32_t n_low[kOrderChunksPerGroup], n_tied[kOrderChunksPerGroup];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t begin = (uint64_t)blockIdx.x * kRowPredRowsPerGroup;
    const uint64_t pivot = take_all ? 0ull : st->pivot;
    uint64_t key[kIters];
    unsigned long long low_bits[kIters], tied_bits[kIters];
#pragma unroll
    for (uint32_t it = 0; it < kIters; ++it) {
        const uint32_t c = it * kWaves + wave;   // the group's 64-row chunk: uniform
        const uint64_t r0 = begin + (uint64_t)c * 64;
        const bool hit = r0 < count && order_hit_bit(hits, r0, lane);
        key[it] = hit ? order_key(vals ? vals[r0 + lane] : 0ll, desc) : 0ull;
        low_bits[it] = __ballot(hit && (take_all || key[it] < pivot));
        tied_bits[it] = __ballot(hit && !take_all && key[it] == pivot);
        if (lane == 0) {
            n_low[c] = (uint32_t)__builtin_popcountll(low_bits[it]);
            n_tied[c] = (uint32_t)__builtin_popcountll(tied_bits[it]);
        }
    }
    __syncthreads();
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) {
            uint32_t lo = 0, ti = 0;
            for (uint32_t c = 0; c < kOrderChunksPerGroup; ++c) { lo += n_low[c]; ti += n_tied[c]; }
            cnt2[(uint64_t)blockIdx.x * 2] = lo;
            cnt2[(uint64_t)blockIdx.x * 2 + 1] = ti;
        }
    } else {
        const uint32_t low0 = first[(uint64_t)blockIdx.x * stride];
        const uint32_t tied0 = take_all ? 0u : first[(uint64_t)blockIdx.x * 2 + 1];
        const uint32_t all_low = take_all ? 0u : first[(uint64_t)n_groups * 2];
        const uint32_t keep = take_all ? 0u : st->remaining;
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (uint32_t it = 0; it < kIters; ++it) {
            const uint32_t c = it * kWaves + wave;
            const bool low = (low_bits[it] >> lane) & 1ull, tied = (tied_bits[it] >> lane) & 1ull;
            if (!low && !tied) continue;
            uint32_t lo = low0, ti = tied0;   // the chunks before this one
            for (uint32_t d = 0; d < c; ++d) { lo += n_low[d]; ti += n_tied[d]; }
            uint64_t at;
            if (low) {
                at = lo + (uint32_t)__builtin_popcountll(low_bits[it] & below);
            } else {
                const uint32_t rank = ti + (uint32_t)__builtin_popcountll(tied_bits[it] & below);
                if (rank >= keep) continue;
                at = (uint64_t)all_low + rank;
            }
            if (at >= n_rec) continue;
            rec[at * 2] = key[it];
            rec[at * 2 + 1] = id_offset + begin + (uint64_t)c * 64 + lane;
        }
    }
}

// ------------------------------------------------------------------ the sort
// rec: P records {key, id}, P a power of two and a multiple of kOrderSortTile.  A work-group takes one tile into LDS and
// runs the network's steps (k, j) for k = k_lo .. k_hi, j = min(k / 2, tile / 2) .. 1: whole sorts of the tile for
// k_lo == 2, the short-distance end of merge k otherwise.  Records at or past n_real read as the pad record.
__global__ __launch_bounds__(kOrderSortThreads) void order_sort_tile_kernel(uint64_t* __restrict__ rec, uint32_t n_real, uint32_t k_lo,
                                                                           uint32_t k_hi) {
    __shared__ uint64_t keys[kOrderSortTile], ids[kOrderSortTile];
    const uint32_t base = blockIdx.x * kOrderSortTile;
    for (uint32_t i = threadIdx.x; i < kOrderSortTile; i += kOrderSortThreads) {
        const bool real = base + i < n_real;
        keys[i] = real ? rec[(uint64_t)(base + i) * 2] : UINT64_MAX;
        ids[i] = real ? rec[(uint64_t)(base + i) * 2 + 1] : UINT64_MAX;
    }
    __syncthreads();
    for (uint32_t k = k_lo; k <= k_hi; k <<= 1) {
        for (uint32_t j = k / 2 < kOrderSortTile / 2 ? k / 2 : kOrderSortTile / 2; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < kOrderSortTile / 2; t += kOrderSortThreads) {
                const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
                const bool swap = order_after(keys[a], ids[a], keys[b], ids[b]) == order_bitonic_up(base + a, k);
                if (swap) {
                    const uint64_t ka = keys[a], ia = ids[a];
                    keys[a] = keys[b]; ids[a] = ids[b];
                    keys[b] = ka; ids[b] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < kOrderSortTile; i += kOrderSortThreads) {
        rec[(uint64_t)(base + i) * 2] = keys[i];
        rec[(uint64_t)(base + i) * 2 + 1] = ids[i];
    }
}

// One step (k, j), j >= kOrderSortTile, in global memory: thread t owns the pair (a, a | j).
__global__ __launch_bounds__(kOrderSortThreads) void order_sort_step_kernel(uint64_t* __restrict__ rec, uint32_t P, uint32_t k, uint32_t j) {
    const uint32_t t = blockIdx.x * kOrderSortThreads + threadIdx.x;
    if (t >= P / 2) return;
    const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
    const uint64_t ka = rec[(uint64_t)a * 2], ia = rec[(uint64_t)a * 2 + 1], kb = rec[(uint64_t)b * 2], ib = rec[(uint64_t)b * 2 + 1];
    if (order_after(ka, ia, kb, ib) == order_bitonic_up(a, k)) {
        rec[(uint64_t)a * 2] = kb; rec[(uint64_t)a * 2 + 1] = ib;
        rec[(uint64_t)b * 2] = ka; rec[(uint64_t)b * 2 + 1] = ia;
    }
}

// The sorted records to the caller's arrays: ids, and (out_vals may be null) the values the keys came from.
__global__ __launch_bounds__(256) void order_emit_kernel(const uint64_t* __restrict__ rec, uint32_t n, bool desc, uint64_t* __restrict__ out_ids,
                                                         int64_t* __restrict__ out_vals) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out_ids[i] = rec[(uint64_t)i * 2 + 1];
    if (out_vals) out_vals[i] = order_value(rec[(uint64_t)i * 2], desc);
}

// ------------------------------------------------------------------ launchers
void launch_order_hits(const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope, uint64_t count,
                       const RowPred& p, bool desc, bool has_cursor, uint64_t ckey, uint64_t cid, uint64_t id_offset, uint32_t* d_hits,
                       uint32_t* d_cnt, hipStream_t s) {
    if (!count) return;
    order_hits_kernel<<<order_groups(count), kOrderThreads, 0, s>>>(d_tags, d_vals, d_labels, d_scope, count, p, desc, has_cursor, ckey, cid,
                                                                    id_offset, d_hits, d_cnt);
}

void launch_order_select(const uint32_t* d_hits, const int64_t* d_vals, uint64_t count, bool desc, uint32_t limit, uint32_t* d_hist,
                         OrderState* d_state, hipStream_t s) {
    if (!count) return;
    order_begin_kernel<<<1, kOrderBins, 0, s>>>(d_hist, d_state, limit);
    for (uint32_t round = 0; round < kOrderRounds; ++round) {
        uint32_t* hist = d_hist + (size_t)round * kOrderBins;
        order_hist_kernel<<<order_groups(count), kOrderThreads, 0, s>>>(d_hits, d_vals, count, desc, round, d_state, hist);
        order_pick_kernel<<<1, 64, 0, s>>>(hist, round, d_state);
    }
}

void launch_order_collect(const uint32_t* d_hits, const int64_t* d_vals, uint64_t count, bool desc, uint64_t id_offset, bool take_all,
                          const OrderState* d_state, uint32_t* d_cnt2, const uint32_t* d_first, uint64_t* d_rec, uint32_t n_rec, hipStream_t s) {
    if (!count) return;
    const uint32_t n_groups = order_groups(count);
    if (take_all) {
        order_collect_kernel<true><<<n_groups, kOrderThreads, 0, s>>>(d_hits, d_vals, count, desc, id_offset, true, nullptr, nullptr, d_first, 1u,
                                                                      n_groups, d_rec, n_rec);
        return;
    }
    order_collect_kernel<false><<<n_groups, kOrderThreads, 0, s>>>(d_hits, d_vals, count, desc, id_offset, false, d_state, d_cnt2, nullptr, 2u,
                                                                   n_groups, nullptr, 0u);
    launch_group_prefix(d_cnt2, n_groups, 2, d_cnt2 + (size_t)n_groups * 2, s);
    order_collect_kernel<true><<<n_groups, kOrderThreads, 0, s>>>(d_hits, d_vals, count, desc, id_offset, false, d_state, nullptr, d_cnt2, 2u,
                                                                  n_groups, d_rec, n_rec);
}

void launch_order_sort(uint64_t* d_rec, uint32_t n, bool desc, uint64_t* d_out_ids, int64_t* d_out_vals, hipStream_t s) {
    if (!n) return;
    const uint32_t P = order_sort_size(n), tiles = P / kOrderSortTile;
    order_sort_tile_kernel<<<tiles, kOrderSortThreads, 0, s>>>(d_rec, n, 2u, kOrderSortTile);
    for (uint32_t k = kOrderSortTile * 2; k <= P; k <<= 1) {
        for (uint32_t j = k / 2; j >= kOrderSortTile; j >>= 1)
            order_sort_step_kernel<<<P / 2 / kOrderSortThreads, kOrderSortThreads, 0, s>>>(d_rec, P, k, j);
        order_sort_tile_kernel<<<tiles, kOrderSortThreads, 0, s>>>(d_rec, P, k, k);
    }
    order_emit_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_rec, n, desc, d_out_ids, d_out_vals);
}

}  // namespace vrod
