// kernels_range.hip -- range search ("every row at least this similar", vrod_range_search) on gfx950.
//
// The batched scan (kernels_mfma*.hip) already is a threshold filter: it appends every row whose FAST score is
// strictly better than a per-query threshold.  With the threshold given by the caller nothing has to be estimated:
//
//   range_prepare_kernel      thr_fast[q] = the caller's threshold moved to the worse side by the fast pass's error
//                             bound and one float further (search_plan.h range_fast_threshold): the lists the scan
//                             fills are a SUPERSET of the answer, the inclusive boundary included
//   range_rescore_cut_kernel  canonical chain of every list entry (rescore_chain.h, the candidate re-score's chain),
//                             comparison with the CALLER's threshold, append of the qualifying rows to the pool
//   range_cut_scores_kernel   canonical route (no finite bound, VROD_PATH_EXACT, the gather route of a narrow filter):
//                             the same comparison and append over a block of canonical scores of all (eligible) rows
//   range_sort_* / range_emit the pool ordered by (query, score best first, id) -- bitonic chunks in LDS and
//                             merge passes by rank, any segment length -- and written as ids and score bits
//
// The pool's counters keep counting when the pool is full: the per-query counts (out_lims) are exact whatever the
// caller's capacity is, and a count-only call stores nothing.
#include "kernels_range.h"
#include "rescore_chain.h"

namespace vrod {

// ------------------------------------------------------------------ fast thresholds
__global__ __launch_bounds__(256) void range_prepare_kernel(const float* __restrict__ thresholds, uint32_t nq, uint32_t nq_pad, int metric,
                                                            int eps_mode, float eps_c, const uint32_t* __restrict__ max_qn2_bits,
                                                            const uint32_t* __restrict__ max_xn2_bits, float* __restrict__ thr_fast,
                                                            uint32_t* __restrict__ canonical) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_pad) return;
    if (q >= nq) {   // padding queries never append
        thr_fast[q] = metric == M_COSINE ? __builtin_huge_valf() : -__builtin_huge_valf();
        canonical[q] = 0u;
        return;
    }
    bool canon = false;
    thr_fast[q] = range_fast_threshold(thresholds[q], metric, eps_mode, eps_c, __uint_as_float(*max_qn2_bits), __uint_as_float(*max_xn2_bits), &canon);
    canonical[q] = canon ? 1u : 0u;
}

void launch_range_prepare(const float* d_thresholds, uint32_t nq, uint32_t nq_pad, int metric, int eps_mode, float eps_c,
                          const uint32_t* d_max_qn2_bits, const uint32_t* d_max_xn2_bits, float* d_thr_fast, uint32_t* d_canonical,
                          hipStream_t s) {
    if (!nq_pad) return;
    range_prepare_kernel<<<(nq_pad + 255) / 256, 256, 0, s>>>(d_thresholds, nq, nq_pad, metric, eps_mode, eps_c, d_max_qn2_bits, d_max_xn2_bits,
                                                             d_thr_fast, d_canonical);
}

// ------------------------------------------------------------------ append to the pool
// The lanes of a wave with `ok` set append one entry each: one pair of atomics per wave (all 64 lanes take part).
// The counters always advance; an entry is stored while its position is inside the pool.
template <int METRIC>
__device__ __forceinline__ void pool_append_wave(const RangePool& pool, bool ok, uint32_t q, float score, uint64_t id) {
    const unsigned long long m = __ballot(ok);
    if (m == 0ull) return;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t lo = 0, hi = 0;
    if (lane == 0) {
        const unsigned long long base = atomicAdd(pool.n_total, (unsigned long long)__builtin_popcountll(m));
        atomicAdd(&pool.per_query[q], (uint32_t)__builtin_popcountll(m));
        lo = (uint32_t)base;
        hi = (uint32_t)(base >> 32);
    }
    lo = __shfl(lo, 0);
    hi = __shfl(hi, 0);
    const uint64_t pos = (((uint64_t)hi << 32) | lo) + (uint64_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (ok && pos < pool.capacity) {
        RangeHit h;
        h.key = ((uint64_t)q << 32) | (uint64_t)(uint32_t)~score_key<METRIC>(score);
        h.id = id;
        pool.pool[pos] = h;
    }
}

template <int METRIC>
__device__ __forceinline__ bool range_qualifies(float score, float threshold) {   // inclusive; a NaN score never does
    return METRIC == M_COSINE ? score >= threshold : score <= threshold;
}

// ------------------------------------------------------------------ re-score and cut
// One wave per block: entries [64 * blockIdx.x, +64) of query blockIdx.y's hit list.
template <typename T, int METRIC>
__global__ __launch_bounds__(64) void range_rescore_cut_kernel(const T* __restrict__ corpus, uint32_t dim, uint32_t ld, const float* __restrict__ q,
                                                               const uint2* __restrict__ lists, const uint32_t* __restrict__ counts, uint32_t cap,
                                                               const float* __restrict__ thresholds, uint32_t q_base, IdMap idmap,
                                                               RangePool pool, uint32_t* __restrict__ max_err) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* q_lds = smem;                       // [ld]
    float* tile = smem + ld;                   // [64][kTileStride]
    const uint32_t lane = threadIdx.x, qi = q_base + blockIdx.y;
    uint32_t n = counts[qi];
    if (n > cap) n = cap;
    const uint32_t slot0 = blockIdx.x * 64u;
    if (slot0 >= n) return;                    // whole wave (single-wave block: no barrier is skipped)
    const float* qrow = q + (uint64_t)qi * ld;
    for (uint32_t i = lane; i < ld; i += 64) q_lds[i] = qrow[i];
    const uint32_t slot = slot0 + lane;
    const bool valid = slot < n;
    const uint2 e = valid ? lists[(uint64_t)qi * cap + slot] : make_uint2(0u, 0u);
    const uint32_t my_row = valid ? e.y : 0u;
    const float canon = canonical_chain_wave<T, METRIC>(corpus, dim, ld, q_lds, tile, my_row, (int)(n - slot0 < 64u ? n - slot0 : 64u));
    float err = valid ? __builtin_fabsf(__uint_as_float(e.x) - canon) : 0.0f;
    if (!(err == err)) err = 0.0f;
    for (int o = 32; o > 0; o >>= 1) err = __builtin_fmaxf(err, __shfl_xor(err, o));
    if (lane == 0 && err > 0.0f) atomicMax(max_err, __float_as_uint(err));
    pool_append_wave<METRIC>(pool, valid && range_qualifies<METRIC>(canon, thresholds[qi]), qi, canon, idmap(my_row));
}

void launch_range_rescore_cut(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q, uint32_t nq,
                              const uint2* d_lists, const uint32_t* d_counts, uint32_t cap, uint32_t max_count, const float* d_thresholds,
                              const IdMap& idmap, const RangePool& pool, uint32_t* d_max_err, hipStream_t s) {
    if (!nq || !max_count) return;
    if (max_count > cap) max_count = cap;
    const size_t lds = ((size_t)ld + 64 * kTileStride) * sizeof(float);
    for (uint32_t q0 = 0; q0 < nq; q0 += 32768u) {   // (grid.y limit)
        const uint32_t nqc = nq - q0 < 32768u ? nq - q0 : 32768u;
        dim3 grid((max_count + 63) / 64, nqc);
#define VROD_RC(TT, MM) \
    range_rescore_cut_kernel<TT, MM><<<grid, 64, lds, s>>>((const TT*)d_corpus, dim, ld, d_q, d_lists, d_counts, cap, d_thresholds, q0, idmap, pool, d_max_err)
        if (dtype == DT_BF16) { if (metric == M_COSINE) VROD_RC(bf16_t, M_COSINE); else VROD_RC(bf16_t, M_L2); }
        else { if (metric == M_COSINE) VROD_RC(float, M_COSINE); else VROD_RC(float, M_L2); }
#undef VROD_RC
    }
}

// ------------------------------------------------------------------ canonical route: cut a block of canonical scores
struct RangeQuerySet { uint32_t qi[8]; };

template <int METRIC>
__global__ __launch_bounds__(256) void range_cut_scores_kernel(const float* __restrict__ scores, uint64_t score_ld, uint64_t n, RangeQuerySet qs,
                                                               uint32_t use_qs, uint32_t q0, const float* __restrict__ thresholds,
                                                               const uint32_t* __restrict__ row_mask, const uint32_t* __restrict__ list,
                                                               IdMap idmap, RangePool pool) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = blockIdx.y;
    const uint32_t q = use_qs ? qs.qi[i & 7u] : q0 + i;
    const bool in = c < n;
    const uint32_t row = in ? (list ? list[c] : (uint32_t)c) : 0u;
    bool ok = in;
    if (ok && row_mask && !list) ok = ((row_mask[row >> 5] >> (row & 31u)) & 1u) == 0u;
    const float sc = in ? scores[(uint64_t)i * score_ld + c] : 0.0f;
    ok = ok && range_qualifies<METRIC>(sc, thresholds[q]);
    pool_append_wave<METRIC>(pool, ok, q, sc, idmap(row));
}

void launch_range_cut_scores(const float* d_scores, uint64_t score_ld, uint64_t n, uint32_t n_queries, const uint32_t* query_index,
                             uint32_t q0, int metric, const float* d_thresholds, const uint32_t* d_row_mask, const uint32_t* d_list,
                             const IdMap& idmap, const RangePool& pool, hipStream_t s) {
    if (!n || !n_queries) return;
    RangeQuerySet qs{};
    if (query_index)
        for (uint32_t i = 0; i < 8; ++i) qs.qi[i] = query_index[i < n_queries ? i : n_queries - 1];
    for (uint32_t i0 = 0; i0 < n_queries; i0 += 32768u) {   // (grid.y limit; a query set has at most 8 entries)
        const uint32_t nqc = n_queries - i0 < 32768u ? n_queries - i0 : 32768u;
        dim3 grid((unsigned)((n + 255) / 256), nqc);
        const float* sc = d_scores + (uint64_t)i0 * score_ld;
        if (metric == M_COSINE)
            range_cut_scores_kernel<M_COSINE><<<grid, 256, 0, s>>>(sc, score_ld, n, qs, query_index ? 1u : 0u, q0 + i0, d_thresholds, d_row_mask, d_list, idmap, pool);
        else
            range_cut_scores_kernel<M_L2><<<grid, 256, 0, s>>>(sc, score_ld, n, qs, query_index ? 1u : 0u, q0 + i0, d_thresholds, d_row_mask, d_list, idmap, pool);
    }
}

// ------------------------------------------------------------------ ordering
// Entries are distinct (an id appears once per query), so a merge by rank needs no tie rule beyond (key, id).
__device__ __forceinline__ bool hit_less(uint64_t ak, uint64_t ai, uint64_t bk, uint64_t bi) { return ak < bk || (ak == bk && ai < bi); }

constexpr uint32_t kRangeSortChunk = 2048, kRangeSortThreads = 256;

// Block b sorts entries [b * kRangeSortChunk, +kRangeSortChunk) in place: bitonic network in LDS, ascending.
__global__ __launch_bounds__(kRangeSortThreads) void range_sort_chunks_kernel(RangeHit* __restrict__ a, uint64_t n) {
    __shared__ uint64_t sk[kRangeSortChunk], si[kRangeSortChunk];
    const uint64_t base = (uint64_t)blockIdx.x * kRangeSortChunk;
    const uint32_t m = (uint32_t)(n - base < kRangeSortChunk ? n - base : kRangeSortChunk);
    uint32_t np2 = 2;
    while (np2 < m) np2 <<= 1;
    for (uint32_t i = threadIdx.x; i < np2; i += kRangeSortThreads) {
        sk[i] = i < m ? a[base + i].key : ~0ull;   // padding sorts last
        si[i] = i < m ? a[base + i].id : ~0ull;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= np2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (np2 >> 1); t += kRangeSortThreads) {
                const uint32_t i = 2 * t - (t & (j - 1));
                const uint32_t l = i + j;
                const bool up = (i & k) == 0;
                const uint64_t xk = sk[i], xi = si[i], yk = sk[l], yi = si[l];
                if (up ? hit_less(yk, yi, xk, xi) : hit_less(xk, xi, yk, yi)) { sk[i] = yk; si[i] = yi; sk[l] = xk; si[l] = xi; }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < m; i += kRangeSortThreads) {
        RangeHit h;
        h.key = sk[i];
        h.id = si[i];
        a[base + i] = h;
    }
}

// One merge pass: the sorted runs of `run` entries of src are merged in pairs into dst.  Entry i goes to its own
// offset in its run plus the number of entries of the sibling run that come before it (binary search).
__global__ __launch_bounds__(256) void range_merge_pass_kernel(const RangeHit* __restrict__ src, RangeHit* __restrict__ dst, uint64_t n, uint64_t run) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RangeHit e = src[i];
    const uint64_t r = i / run, my0 = r * run;
    const bool left = (r & 1ull) == 0ull;
    const uint64_t pair0 = left ? my0 : my0 - run;
    const uint64_t sib0 = left ? my0 + run : my0 - run;
    uint64_t lo = sib0 < n ? sib0 : n;
    uint64_t hi = sib0 + run < n ? sib0 + run : n;
    if (hi < lo) hi = lo;
    const uint64_t first = lo;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const RangeHit x = src[mid];
        // left run: sibling entries strictly before e; right run: sibling entries not after e
        const bool before = left ? hit_less(x.key, x.id, e.key, e.id) : !hit_less(e.key, e.id, x.key, x.id);
        if (before) lo = mid + 1; else hi = mid;
    }
    dst[pair0 + (i - my0) + (lo - first)] = e;
}

RangeHit* launch_range_sort(RangeHit* d_a, RangeHit* d_b, uint64_t n, hipStream_t s) {
    if (!n) return d_a;
    range_sort_chunks_kernel<<<(unsigned)((n + kRangeSortChunk - 1) / kRangeSortChunk), kRangeSortThreads, 0, s>>>(d_a, n);
    RangeHit *cur = d_a, *other = d_b;
    for (uint64_t run = kRangeSortChunk; run < n; run <<= 1) {
        range_merge_pass_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(cur, other, n, run);
        RangeHit* t = cur; cur = other; other = t;
    }
    return cur;
}

__global__ __launch_bounds__(256) void range_emit_kernel(const RangeHit* __restrict__ sorted, uint64_t n, int metric, uint64_t* __restrict__ out_ids,
                                                         float* __restrict__ out_scores) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RangeHit h = sorted[i];
    out_ids[i] = h.id;
    out_scores[i] = key_to_score_rt(~(uint32_t)(h.key & 0xFFFFFFFFull), metric);
}

void launch_range_emit(const RangeHit* d_sorted, uint64_t n, int metric, uint64_t* d_out_ids, float* d_out_scores, hipStream_t s) {
    if (!n) return;
    range_emit_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_sorted, n, metric, d_out_ids, d_out_scores);
}

}  // namespace vrod
