// kernels_centroid.hip -- the device side of group centroids (vrod_index_centroids_where; gfx950): the exact, order-free
// vector sum or mean of every group of the rows a row predicate matches, the groups being labels or value buckets.
//
// The reference has no attributes beside a row (src/database/mod.rs), so it has no groups to average; "the embedding of
// a document as the mean of its chunks" needs the one aggregate kernels_aggregate.hip cannot give, the vectors.
//
// A float sum is not associative, so the sum is defined on integers (centroid_plan.h): every element is quantised to an
// int64 at one scale per call, the group's sum is an int64 that cannot wrap, and one conversion at the end gives the
// float.  Integer adds commute, so partial sums may be folded in registers and land by atomics in any order without
// changing a bit -- the argument of kernels_aggregate.hip, applied to the vectors.
//
// The groups, their counts and their table come from the aggregation pass, the matching rows from the hit bitmap of
// launch_rowpred_hits.  Four launches, the walks over the geometry of kernels_rowpred.hip (work-group b owns rows
// [b * R, (b + 1) * R), R = kRowPredRowsPerGroup, and reads their 64 hit words):
//   ranks  : the host has ordered the groups; thread g finds key g's slot in the aggregation's table and writes g there;
//   max    : (L2 and IP handles) the largest |x| bits among the considered rows, an integer max;
//   add    : the hot path, one read of every considered row.  The work-group lists its hits ascending in LDS with each
//            row's rank (its key looked up in the table), teams of lanes take contiguous parts of the list, a lane owns a
//            16-byte piece of the row and keeps its int64 sums in registers while the rank does not change; a change
//            flushes them with 64-bit integer atomic adds whose value nobody reads.  Contiguous rows of one document
//            cost one flush per team, scattered labels one atomic per element: slower, and the same bits;
//   finish : sum or mean of every (group, element) as fp32 at the caller's stride.
#include "centroid_plan.h"
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

#define CEN_RLX __ATOMIC_RELAXED
#define CEN_DEV __HIP_MEMORY_SCOPE_AGENT

// The slot of `key` in the aggregation's table, read-only: the pass has ended.  g.slots + 1: not there.
__device__ __forceinline__ uint64_t centroid_find_slot(const AggTable& g, int64_t key) {
    if (key == kAggEmptyKey) return g.slots;
    uint64_t s = agg_home(key, g.slots);
    for (uint64_t i = 0; i < g.slots; ++i) {
        const int64_t cur = g.key[s];
        if (cur == key) return s;
        if (cur == kAggEmptyKey) break;
        s = (s + 1) & (g.slots - 1);
    }
    return g.slots + 1;
}

// rank[slot of keys[g]] = g.  Every other entry keeps the kCentroidNoRank the host filled in.
__global__ __launch_bounds__(256) void centroid_ranks_kernel(AggTable g, const int64_t* __restrict__ keys, uint32_t n_groups,
                                                             uint32_t* __restrict__ rank) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_groups) return;
    const uint64_t s = centroid_find_slot(g, keys[i]);
    if (s <= g.slots) rank[s] = i;
}

// The 16-byte piece `piece` of row r.  A row is ld elements of 128-byte granularity, so every piece below ld lies in it.
__device__ __forceinline__ u32x4_t centroid_load(const char* __restrict__ corpus, size_t row_bytes, uint64_t r, uint32_t piece) {
    return *(const u32x4_t*)(corpus + r * row_bytes + (size_t)piece * 16);
}
// Element e of a piece as fp32 bits: 8 bf16 (the low half of a word first) or 4 fp32.
template <typename T>
__device__ __forceinline__ uint32_t centroid_elem_bits(const u32x4_t& v, int e) {
    if constexpr (sizeof(T) == 2) return (e & 1) ? (v[e >> 1] & 0xFFFF0000u) : (v[e >> 1] << 16);
    else return v[e];
}

// ADD = false: max_bits[0] = max(max_bits[0], bits(x) & 0x7fffffff) over the elements below dim of the rows whose hit
// bit is set.  ADD = true: acc[rank(row)][j] += centroid_quantise(x, scale) over the same elements; a row whose key has
// no rank below n_groups adds nothing (the aggregation listed every key, so there is none).
template <typename T, bool ADD>
__global__ __launch_bounds__(kCentroidThreads) void centroid_walk_kernel(const char* __restrict__ corpus, uint32_t dim, uint32_t ld,
                                                                         const uint32_t* __restrict__ hits, uint64_t n_words, uint64_t count,
                                                                         uint32_t by, const int64_t* __restrict__ vals,
                                                                         const uint32_t* __restrict__ labels, int64_t width, AggTable g,
                                                                         const uint32_t* __restrict__ rank, uint32_t n_groups, int32_t scale,
                                                                         unsigned long long* __restrict__ acc, uint32_t* __restrict__ max_bits) {
    constexpr int EPP = 16 / (int)sizeof(T);
    constexpr uint32_t kWords = kRowPredRowsPerGroup / 32;   // 64: a hit word per lane of the first wave
    __shared__ uint32_t word[kWords];
    __shared__ uint32_t base[kWords + 1];
    __shared__ uint16_t lrow[kRowPredRowsPerGroup];
    __shared__ uint32_t lrank[ADD ? kRowPredRowsPerGroup : 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t begin = (uint64_t)blockIdx.x * kRowPredRowsPerGroup;
    // the hit words and their exclusive prefix: where each word's rows start in the list
    if (tid < kWords) {
        const uint64_t w = (uint64_t)blockIdx.x * kWords + tid;
        const uint32_t bits = w < n_words ? hits[w] : 0u;
        const uint32_t mine = (uint32_t)__builtin_popcount(bits);
        uint32_t upto = mine;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(upto, d);
            if (tid >= d) upto += o;
        }
        word[tid] = bits;
        base[tid] = upto - mine;
        if (tid == kWords - 1) base[kWords] = upto;
    }
    __syncthreads();
    const uint32_t n = base[kWords];
    if (!n) return;   // the whole work-group
    // the list, ascending: thread t owns the 8 rows of byte t & 3 of word t >> 2
    {
        const uint32_t w = tid >> 2, shift = (tid & 3u) * 8u;
        uint32_t at = base[w] + (uint32_t)__builtin_popcount(word[w] & ((1u << shift) - 1u));
        uint32_t mine = (word[w] >> shift) & 0xFFu;
        while (mine) {
            const uint32_t off = tid * 8u + (uint32_t)__builtin_ctz(mine);
            mine &= mine - 1u;
            const uint64_t r = begin + off;
            if (r >= count) break;   // (no hit bit is set past the count)
            lrow[at] = (uint16_t)off;
            if constexpr (ADD) {
                const int64_t key = agg_key(by, labels ? labels[r] : 0u, vals ? vals[r] : 0ll, width);
                const uint64_t s = centroid_find_slot(g, key);
                lrank[at] = s <= g.slots ? rank[s] : kCentroidNoRank;
            }
            ++at;
        }
    }
    __syncthreads();
    // teams of TL lanes, a lane a piece; team t walks entries [t * per, (t + 1) * per) of the list
    const uint32_t pieces = centroid_pieces(dim, EPP), TL = centroid_team(pieces), teams = kCentroidThreads / TL;
    const uint32_t tl = tid & (TL - 1u), team = tid / TL;
    const uint32_t per = (n + teams - 1u) / teams;
    const uint32_t i0 = team * per < n ? team * per : n, i1 = i0 + per < n ? i0 + per : n;
    const size_t row_bytes = (size_t)ld * sizeof(T);
    uint32_t mx = 0u;
    for (uint32_t piece = tl; piece < pieces; piece += TL) {
        const uint32_t j0 = piece * EPP;
        long long sum[EPP];
#pragma unroll
        for (int e = 0; e < EPP; ++e) sum[e] = 0ll;
        uint32_t cur = kCentroidNoRank;
        auto flush = [&]() {
            if (cur >= n_groups) return;
            unsigned long long* dst = acc + (uint64_t)cur * dim + j0;
#pragma unroll
            for (int e = 0; e < EPP; ++e)
                if (j0 + e < dim && sum[e] != 0ll) (void)__hip_atomic_fetch_add(dst + e, (unsigned long long)sum[e], CEN_RLX, CEN_DEV);
        };
        for (uint32_t i = i0; i < i1; i += kCentroidInFlight) {
            u32x4_t v[kCentroidInFlight];
#pragma unroll
            for (uint32_t u = 0; u < kCentroidInFlight; ++u)   // the loads of several rows first, so that they overlap
                if (i + u < i1) v[u] = centroid_load(corpus, row_bytes, begin + lrow[i + u], piece);
#pragma unroll
            for (uint32_t u = 0; u < kCentroidInFlight; ++u) {
                if (i + u >= i1) break;
                if constexpr (ADD) {
                    const uint32_t rk = lrank[i + u];
                    if (rk != cur) {
                        flush();
                        cur = rk;
#pragma unroll
                        for (int e = 0; e < EPP; ++e) sum[e] = 0ll;
                    }
#pragma unroll
                    for (int e = 0; e < EPP; ++e)   // the padding between dim and ld is nobody's element: it is not even quantised
                        if (j0 + e < dim) sum[e] += (long long)centroid_quantise(centroid_elem_bits<T>(v[u], e), scale);
                } else {
#pragma unroll
                    for (int e = 0; e < EPP; ++e) {
                        const uint32_t a = centroid_elem_bits<T>(v[u], e) & 0x7FFFFFFFu;
                        if (j0 + e < dim && a > mx) mx = a;
                    }
                }
            }
        }
        if constexpr (ADD) flush();
    }
    if constexpr (!ADD) {
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = __shfl_xor(mx, o);
            mx = other > mx ? other : mx;
        }
        if ((tid & 63u) == 0u && mx) (void)__hip_atomic_fetch_max(max_bits, mx, CEN_RLX, CEN_DEV);
    }
}

// out[g * stride + j] = the sum or the mean of acc[g][j], j < dim: the elements between dim and the stride are not touched.
__global__ __launch_bounds__(256) void centroid_finish_kernel(const unsigned long long* __restrict__ acc, const uint64_t* __restrict__ counts,
                                                              uint32_t n_groups, uint32_t dim, int32_t scale, bool sums,
                                                              float* __restrict__ out, uint64_t stride) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)n_groups * dim) return;
    const uint64_t grp = i / dim;
    const uint32_t j = (uint32_t)(i - grp * dim);
    const int64_t S = (int64_t)acc[i];
    out[grp * stride + j] = sums ? centroid_sum_value(S, scale) : centroid_mean_value(S, counts[grp], scale);
}

// ------------------------------------------------------------------ launchers
void launch_centroid_ranks(const AggTable& g, const int64_t* d_keys, uint32_t n_groups, uint32_t* d_rank, hipStream_t s) {
    if (!n_groups) return;
    centroid_ranks_kernel<<<(n_groups + 255) / 256, 256, 0, s>>>(g, d_keys, n_groups, d_rank);
}

void launch_centroid_max(const void* d_corpus, int dtype, uint32_t dim, uint32_t ld, const uint32_t* d_hits, uint64_t count, uint32_t* d_max_bits,
                         hipStream_t s) {
    if (!count) return;
    const uint32_t groups = centroid_groups(count);
    const uint64_t n_words = row_pred_hit_words(count);
    const AggTable none{};
    if (dtype == DT_BF16)
        centroid_walk_kernel<bf16_t, false><<<groups, kCentroidThreads, 0, s>>>((const char*)d_corpus, dim, ld, d_hits, n_words, count, 0u, nullptr, nullptr,
                                                                               1, none, nullptr, 0u, 0, nullptr, d_max_bits);
    else
        centroid_walk_kernel<float, false><<<groups, kCentroidThreads, 0, s>>>((const char*)d_corpus, dim, ld, d_hits, n_words, count, 0u, nullptr, nullptr, 1,
                                                                              none, nullptr, 0u, 0, nullptr, d_max_bits);
}

void launch_centroid_add(const void* d_corpus, int dtype, uint32_t dim, uint32_t ld, const uint32_t* d_hits, uint64_t count, uint32_t by,
                         const int64_t* d_vals, const uint32_t* d_labels, int64_t width, const AggTable& g, const uint32_t* d_rank,
                         uint32_t n_groups, int32_t scale, int64_t* d_acc, hipStream_t s) {
    if (!count || !n_groups) return;
    const uint32_t groups = centroid_groups(count);
    const uint64_t n_words = row_pred_hit_words(count);
    if (dtype == DT_BF16)
        centroid_walk_kernel<bf16_t, true><<<groups, kCentroidThreads, 0, s>>>((const char*)d_corpus, dim, ld, d_hits, n_words, count, by, d_vals, d_labels,
                                                                              width, g, d_rank, n_groups, scale, (unsigned long long*)d_acc, nullptr);
    else
        centroid_walk_kernel<float, true><<<groups, kCentroidThreads, 0, s>>>((const char*)d_corpus, dim, ld, d_hits, n_words, count, by, d_vals, d_labels,
                                                                             width, g, d_rank, n_groups, scale, (unsigned long long*)d_acc, nullptr);
}

void launch_centroid_finish(const int64_t* d_acc, const uint64_t* d_counts, uint32_t n_groups, uint32_t dim, int32_t scale, bool sums, float* d_out,
                            uint64_t stride, hipStream_t s) {
    if (!n_groups) return;
    const uint64_t total = (uint64_t)n_groups * dim;
    centroid_finish_kernel<<<(uint32_t)((total + 255) / 256), 256, 0, s>>>((const unsigned long long*)d_acc, d_counts, n_groups, dim, scale, sums, d_out,
                                                                          stride);
}

}  // namespace vrod
