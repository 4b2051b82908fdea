// kernels_multivec.hip -- the device side of a multi-vector search (vrod_search_multivec, gfx950): a query is a set of
// vectors, a document the rows of one label, S(q, L) = the fp32 sum over the query's vectors, in order, of the best
// canonical score M(t, L) of vector t over the label's eligible rows.
//
// Dense route (every document of the handle):
//   multivec_fold_kernel      canonical score blocks [vectors][rows] -> best[vector][document], an integer atomic maximum
//                             of an order-preserving image of the score.  The image keeps two values below every real
//                             score: 0 = no eligible row yet, 1 = only NaN scores so far -- an eligible row's own score
//                             may be the worst there is (-inf under IP, a NaN), and a document without an eligible row
//                             must be absent, not last (kernels_group.hip group_mask_kernel has the same reason).
//   multivec_sum_kernel       S[document] += M(t, document), vector after vector, one rounding per add, and the bitmap
//                             of the absent documents the select chain takes as its row mask.
// Candidate route (the labels of the rows in the query's certified top-k1 lists):
//   multivec_candidates_kernel  one work-group per query: the distinct labels of its lists' rows (the hash-table idiom
//                             of group_dedupe_kernel, in global memory: a query has up to 256 lists), whether a list
//                             came back short or holds a non-finite score, and U = the fl-sum of the lists' last scores.
//   multivec_slot_best_kernel M(t, L) of every score slot of the segmented launch (one wave per slot).
//   multivec_pair_sum_kernel  S of every (query, candidate) pair from its vectors' slots, in vector order.
// Both routes end in the select chain over S and multivec_output_kernel: sorted keys -> labels, scores, found.
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "multivec_plan.h"

namespace vrod {

constexpr uint32_t kMvEmpty = 0xFFFFFFFFu;
constexpr uint32_t kMvKeyAbsent = 0u, kMvKeyNan = 1u;   // below the key of every number (-inf / +inf: 0x007FFFFF)

__device__ __forceinline__ uint32_t mv_key(float s, int form) {
    const uint32_t k = score_key_rt(s, form);
    return k ? k : kMvKeyNan;
}
__device__ __forceinline__ float mv_score(uint32_t key, int form) {
    return key <= kMvKeyNan ? __uint_as_float(kScoreNoneBits) : key_to_score_rt(key, form);
}

// scores [g][score_ld]: row r < n_rows of vector i.  best [g][n_docs], zeroed by the caller.  rank == null: one document.
__global__ __launch_bounds__(256) void multivec_fold_kernel(const float* __restrict__ scores, uint64_t score_ld, uint32_t g, uint64_t n_rows,
                                                            const uint32_t* __restrict__ rank, const uint32_t* __restrict__ mask, int form,
                                                            uint32_t* __restrict__ best, uint64_t n_docs) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256) {
        if (mask && ((mask[r >> 5] >> (r & 31u)) & 1u)) continue;
        const uint64_t d = rank ? rank[r] : 0u;
        if (d >= n_docs) continue;   // (never: the ranks are below n_docs by construction)
        for (uint32_t i = 0; i < g; ++i) {
            const uint32_t key = mv_key(scores[(uint64_t)i * score_ld + r], form);
            uint32_t* b = best + (uint64_t)i * n_docs + d;
            if (*b < key) atomicMax(b, key);
        }
    }
}

// S[d] = (first ? +0 : S[d]) + M(0, d) + ... + M(g - 1, d), left to right.  absent != null: bit d = document d has no
// eligible row (the documents at and beyond n_docs of the last word included).
__global__ __launch_bounds__(256) void multivec_sum_kernel(const uint32_t* __restrict__ best, uint32_t g, uint64_t n_docs, int form, int first,
                                                           float* __restrict__ S, uint32_t* __restrict__ absent) {
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool gone = true;
    if (d < n_docs) {
        float s = first ? 0.0f : S[d];
        gone = best[d] == kMvKeyAbsent;
        for (uint32_t i = 0; i < g; ++i) s = s + mv_score(best[(uint64_t)i * n_docs + d], form);
        S[d] = s;
    }
    if (absent) {   // (uniform: the grid covers whole waves)
        const unsigned long long m = __ballot(gone);
        const uint32_t lane = threadIdx.x & 63u;
        const uint64_t w = d >> 5;
        if (lane == 0 && (w << 5) < n_docs) absent[w] = (uint32_t)m;
        if (lane == 32 && (w << 5) < n_docs) absent[w] = (uint32_t)(m >> 32);
    }
}

// ------------------------------------------------------------------ candidate route
__device__ __forceinline__ uint32_t mv_hash(uint32_t label, uint32_t shift) { return (label * 2654435761u) >> shift; }

// Block q: the lists of query qs[q] (ids / scores [vectors][k1], best first, unfilled slots last).  lab [entries] and
// table [slots] (all kMvEmpty) are the query's own regions of global memory.  cand + ent_off receives the distinct labels
// (no order), count[q] how many; flags[q] bit 0 = a list came back short, bit 1 = a list holds a non-finite score;
// U[q] = theta_0 + theta_1 + ... from +0, theta_t = the last score of list t (meaningful while no list is short).
__global__ __launch_bounds__(256) void multivec_candidates_kernel(const uint64_t* __restrict__ ids, const float* __restrict__ scores, uint32_t k1,
                                                                  const uint32_t* __restrict__ labels, uint64_t id_offset,
                                                                  const MultivecQuery* __restrict__ qs, uint32_t* lab, uint32_t* table,
                                                                  uint32_t* __restrict__ cand,
                                                                  uint32_t* __restrict__ count, uint32_t* __restrict__ flags,
                                                                  float* __restrict__ U) {
    __shared__ uint32_t n_out, fl;
    const MultivecQuery Q = qs[blockIdx.x];
    const uint32_t tid = threadIdx.x, entries = Q.m * k1, slot_mask = Q.slots - 1;
    const uint64_t* my_ids = ids + (uint64_t)Q.v0 * k1;
    const float* my_sc = scores + (uint64_t)Q.v0 * k1;
    uint32_t* my_lab = lab + Q.ent_off;
    uint32_t* my_tab = table + Q.tab_off;
    if (tid == 0) { n_out = 0u; fl = 0u; }
    __syncthreads();
    uint32_t f = 0;
    for (uint32_t i = tid; i < entries; i += 256) {
        const uint64_t id = my_ids[i];
        const bool real = id != UINT64_MAX;
        my_lab[i] = real && labels ? labels[id - id_offset] : 0u;
        if (!real) f |= 1u;
        else if ((__float_as_uint(my_sc[i]) & 0x7F800000u) == 0x7F800000u) f |= 2u;
    }
    if (f) atomicOr(&fl, f);
    __syncthreads();
    for (uint32_t i = tid; i < entries; i += 256) {
        if (my_ids[i] == UINT64_MAX) continue;
        const uint32_t label = my_lab[i];
        uint32_t h = mv_hash(label, Q.shift);
        for (;;) {   // (the table keeps empty slots: every probe sequence ends)
            const uint32_t old = atomicCAS(&my_tab[h], kMvEmpty, i);
            if (old == kMvEmpty) break;
            if (my_lab[old] == label) { atomicMin(&my_tab[h], i); break; }
            h = (h + 1) & slot_mask;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < entries; i += 256) {
        if (my_ids[i] == UINT64_MAX) continue;
        const uint32_t label = my_lab[i];
        uint32_t h = mv_hash(label, Q.shift);
        for (;;) {
            const uint32_t j = my_tab[h];
            if (j == kMvEmpty) break;   // (never: the label was inserted above)
            if (my_lab[j] == label) { if (j == i) cand[Q.ent_off + atomicAdd(&n_out, 1u)] = label; break; }
            h = (h + 1) & slot_mask;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float u = 0.0f;
        for (uint32_t t = 0; t < Q.m; ++t) u = u + my_sc[(uint64_t)t * k1 + k1 - 1];
        U[blockIdx.x] = u;
        count[blockIdx.x] = n_out;
        flags[blockIdx.x] = fl;
    }
}

// Slot s < n_slots of a score chunk [n_slots][score_ld]: M[s] = the best of its first len[s] scores, a NaN losing to any
// number (NaN when every score is one, or the slot has no row).  One wave per slot.
__global__ __launch_bounds__(256) void multivec_slot_best_kernel(const float* __restrict__ scores, uint64_t score_ld, uint32_t n_slots,
                                                                 const uint32_t* __restrict__ len, int form, float* __restrict__ M) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_slots) return;
    const float* row = scores + (uint64_t)s * score_ld;
    const uint32_t n = len[s];
    uint32_t best = 0;
    for (uint32_t c = lane; c < n; c += 64) {
        const uint32_t key = mv_key(row[c], form);
        best = key > best ? key : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t v = __shfl_xor(best, o);
        best = v > best ? v : best;
    }
    if (lane == 0) M[s] = mv_score(best, form);
}

// Pair p: S = M[slot[p]] + M[slot[p] + 1] + ... (m[p] vectors, from +0, left to right) -> out[dst[p]].
__global__ __launch_bounds__(256) void multivec_pair_sum_kernel(const float* __restrict__ M, const uint32_t* __restrict__ slot,
                                                                const uint32_t* __restrict__ m, const uint64_t* __restrict__ dst,
                                                                uint32_t n_pairs, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const float* v = M + slot[p];
    float s = 0.0f;
    for (uint32_t t = 0; t < m[p]; ++t) s = s + v[t];
    out[dst[p]] = s;
}

// Block i: the sorted keys of result row i (keys + i * key_ld, kp of them, best first, 0 = none) -> row q = qidx[i] (i
// itself without qidx) of the outputs [..][k]: label = table[tab_off[i] + column] (tab_off == null: 0), score = S, the
// slots beyond the keys (label 0, NaN); found[q] = the filled slots; kth[i] (may be null) = the score of slot k - 1.
__global__ __launch_bounds__(256) void multivec_output_kernel(const uint64_t* __restrict__ keys, uint64_t key_ld, uint32_t kp, int form, uint32_t k,
                                                             const uint32_t* __restrict__ table, const uint32_t* __restrict__ tab_off,
                                                             const uint32_t* __restrict__ qidx, uint32_t* __restrict__ out_labels,
                                                             float* __restrict__ out_scores, uint32_t* __restrict__ found,
                                                             float* __restrict__ kth) {
    const uint32_t i = blockIdx.x;
    const uint64_t q = qidx ? qidx[i] : i;
    const uint64_t* my = keys + (uint64_t)i * key_ld;
    const uint32_t* tab = table + (tab_off ? tab_off[i] : 0u);
    if (threadIdx.x == 0 && (kp == 0 || my[0] == 0ull)) found[q] = 0u;
    for (uint32_t j = threadIdx.x; j < k; j += 256) {
        const uint64_t key = j < kp ? my[j] : 0ull;
        const float s = key ? key_to_score_rt(key_skey(key), form) : __uint_as_float(kScoreNoneBits);
        out_labels[q * k + j] = key ? tab[key_row(key)] : 0u;
        out_scores[q * k + j] = s;
        if (key && (j + 1 == k || j + 1 >= kp || my[j + 1] == 0ull)) found[q] = j + 1;
        if (kth && j + 1 == k) kth[i] = s;
    }
}

// ------------------------------------------------------------------ launchers
void launch_multivec_fold(const float* d_scores, uint64_t score_ld, uint32_t g, uint64_t n_rows, const uint32_t* d_rank, const uint32_t* d_mask,
                          int metric, uint32_t* d_best, uint64_t n_docs, hipStream_t s) {
    if (!n_rows || !g) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_rows + 255) / 256, 65536);
    multivec_fold_kernel<<<grid, 256, 0, s>>>(d_scores, score_ld, g, n_rows, d_rank, d_mask, metric, d_best, n_docs);
}

void launch_multivec_sum(const uint32_t* d_best, uint32_t g, uint64_t n_docs, int metric, bool first, float* d_S, uint32_t* d_absent,
                         hipStream_t s) {
    if (!n_docs) return;
    multivec_sum_kernel<<<(unsigned)((n_docs + 255) / 256), 256, 0, s>>>(d_best, g, n_docs, metric, first ? 1 : 0, d_S, d_absent);
}

void launch_multivec_candidates(const uint64_t* d_ids, const float* d_scores, uint32_t k1, const uint32_t* d_labels, uint64_t id_offset,
                                const MultivecQuery* d_queries, uint32_t nq, uint32_t* d_lab, uint32_t* d_table, uint32_t* d_cand, uint32_t* d_count,
                                uint32_t* d_flags, float* d_U, hipStream_t s) {
    if (!nq) return;
    multivec_candidates_kernel<<<nq, 256, 0, s>>>(d_ids, d_scores, k1, d_labels, id_offset, d_queries, d_lab, d_table, d_cand,
                                                  d_count, d_flags, d_U);
}

void launch_multivec_slot_best(const float* d_scores, uint64_t score_ld, uint32_t n_slots, const uint32_t* d_len, int metric, float* d_M,
                               hipStream_t s) {
    if (!n_slots) return;
    multivec_slot_best_kernel<<<(n_slots + 3) / 4, 256, 0, s>>>(d_scores, score_ld, n_slots, d_len, metric, d_M);
}

void launch_multivec_pair_sum(const float* d_M, const uint32_t* d_slot, const uint32_t* d_m, const uint64_t* d_dst, uint32_t n_pairs, float* d_out,
                              hipStream_t s) {
    if (!n_pairs) return;
    multivec_pair_sum_kernel<<<(n_pairs + 255) / 256, 256, 0, s>>>(d_M, d_slot, d_m, d_dst, n_pairs, d_out);
}

void launch_multivec_output(const uint64_t* d_keys, uint64_t key_ld, uint32_t kp, uint32_t n_rows, int metric, uint32_t k, const uint32_t* d_table,
                            const uint32_t* d_tab_off, const uint32_t* d_qidx, uint32_t* d_out_labels, float* d_out_scores, uint32_t* d_found,
                            float* d_kth, hipStream_t s) {
    if (!n_rows) return;
    multivec_output_kernel<<<n_rows, 256, 0, s>>>(d_keys, key_ld, kp, metric, k, d_table, d_tab_off, d_qidx, d_out_labels, d_out_scores, d_found,
                                                  d_kth);
}

}  // namespace vrod
