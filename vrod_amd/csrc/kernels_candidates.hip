// kernels_candidates.hip -- candidate-list searches (vrod_search_candidates, vrod_score_candidates) on gfx950.
//
// The caller hands every query an unordered list of ids: repeats, deleted rows, disallowed rows and ids that were never
// rows are all allowed in it.  Three steps turn such lists into what the rest of the library works on:
//
//   cand_resolve_kernel      one thread per list entry: id -> local row, or kCandNoRow when the id is no current row
//                            or its bit is set in the handle's row mask (tombstones | ~filter)
//   cand_sort_unique_kernel  one work-group per query: its resolved rows sorted ascending in LDS (bitonic network of the
//                            list's own power of two), the entries that repeat their predecessor or name no row dropped,
//                            the survivors written to the query's segment of the list buffer and counted -- the
//                            ascending, duplicate-free segment the segmented driver scores (vrod_index.hip run_segments)
//   cand_score_kernel        the score form: the canonical chain (rescore_chain.h) of every entry of the resolved,
//                            UNSORTED lists, one (query, entry) pair per lane, written at the entry's own position
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "rescore_chain.h"

namespace vrod {

static_assert((size_t)kCandMaxList * sizeof(uint32_t) == 64 * 1024, "one list must fill exactly the 64 KB of LDS its work-group sorts it in");
static_assert(kCandClassCap[kCandClasses - 1] == kCandMaxList, "the largest sort class holds the longest list");

// ------------------------------------------------------------------ ids -> rows
__global__ __launch_bounds__(256) void cand_resolve_kernel(const uint64_t* __restrict__ ids, uint32_t n, uint64_t count, uint64_t id_offset,
                                                           const uint32_t* __restrict__ row_mask, uint32_t* __restrict__ rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t id = ids[i];
    uint32_t r = kCandNoRow;
    if (id != UINT64_MAX && id >= id_offset && id - id_offset < count) {
        const uint32_t row = (uint32_t)(id - id_offset);
        if (!row_mask || !((row_mask[row >> 5] >> (row & 31u)) & 1u)) r = row;
    }
    rows[i] = r;
}

void launch_cand_resolve(const uint64_t* d_ids, uint32_t n, uint64_t count, uint64_t id_offset, const uint32_t* d_row_mask, uint32_t* d_rows,
                         hipStream_t s) {
    if (!n) return;
    cand_resolve_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_ids, n, count, id_offset, d_row_mask, d_rows);
}

// ------------------------------------------------------------------ sort + unique
// Work-group b takes query qidx[b]: entries [lims[q], lims[q + 1]) of `rows`, at most CAP of them (the query's class,
// candidates_plan.h).  The list is padded with kCandNoRow -- which sorts last -- to its own power of two and only that
// network runs.  Afterwards thread t owns the CAP / NT consecutive sorted entries from t * CAP / NT on: it keeps them in
// registers, so that the LDS the list lay in can carry the block's prefix sum, and writes its survivors in order.
template <uint32_t NT, uint32_t CAP>
__global__ __launch_bounds__(NT) void cand_sort_unique_kernel(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ lims,
                                                              const uint32_t* __restrict__ qidx, uint32_t* __restrict__ lists,
                                                              uint32_t* __restrict__ len) {
    extern __shared__ __attribute__((aligned(16))) uint32_t a[];   // [CAP]
    constexpr uint32_t R = CAP / NT;
    static_assert(R % 4 == 0 && NT % 64 == 0 && NT / 64 <= CAP, "a thread owns whole 16-B units; the wave sums fit the list's LDS");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = qidx[blockIdx.x];
    const uint32_t base = lims[q];
    uint32_t n = lims[q + 1] - base;
    if (n > CAP) n = CAP;   // (never: the host put the query into a class that holds it)
    uint32_t np2 = n ? 1u : 0u;
    while (np2 < n) np2 <<= 1;
    for (uint32_t i = tid; i < np2; i += NT) a[i] = i < n ? rows[base + i] : kCandNoRow;
    __syncthreads();
    for (uint32_t k = 2; k <= np2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (np2 >> 1); t += NT) {
                const uint32_t i = 2 * t - (t & (j - 1));
                const uint32_t l = i + j;
                const bool up = (i & k) == 0;
                const uint32_t x = a[i], y = a[l];
                if ((x > y) == up) { a[i] = y; a[l] = x; }
            }
            __syncthreads();
        }
    }
    // this thread's entries; beyond the network everything is padding (what the LDS holds there was never written)
    const uint32_t i0 = tid * R;
    uint32_t v[R];
#pragma unroll
    for (uint32_t u = 0; u < R; u += 4) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(a + i0 + u);
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) v[u + e] = i0 + u + e < np2 ? w[e] : kCandNoRow;
    }
    uint32_t prev = tid && i0 - 1 < np2 ? a[i0 - 1] : kCandNoRow;   // (entry 0 has no predecessor: a row there survives)
    uint32_t keep = 0, c = 0;                                       // bit e: entry e survives
#pragma unroll
    for (uint32_t e = 0; e < R; ++e) {
        if (v[e] != kCandNoRow && v[e] != prev) { keep |= 1u << e; ++c; }
        prev = v[e];
    }
    __syncthreads();   // every thread holds its entries: the LDS is free
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63) a[wave] = incl;
    __syncthreads();
    uint32_t before = incl - c, total = 0;
    for (uint32_t w = 0; w < NT / 64; ++w) {
        const uint32_t s = a[w];
        if (w < wave) before += s;
        total += s;
    }
    uint32_t* o = lists + base + before;   // before + c <= n: the segment is never longer than the list
#pragma unroll
    for (uint32_t e = 0; e < R; ++e)
        if ((keep >> e) & 1u) *o++ = v[e];
    if (tid == 0) len[q] = total;
}

void launch_cand_sort_unique(const uint32_t* d_rows, const uint32_t* d_lims, const uint32_t* d_qidx, uint32_t n_queries, uint32_t sort_class,
                             uint32_t* d_lists, uint32_t* d_len, hipStream_t s) {
    if (!n_queries) return;
#define VROD_CS(C) \
    cand_sort_unique_kernel<kCandClassThreads[C], kCandClassCap[C]><<<n_queries, kCandClassThreads[C], kCandClassCap[C] * 4, s>>>(d_rows, d_lims, d_qidx, d_lists, d_len)
    switch (sort_class) {
        case 0: VROD_CS(0); break;
        case 1: VROD_CS(1); break;
        default: VROD_CS(2); break;
    }
#undef VROD_CS
}

// ------------------------------------------------------------------ the score form
// One wave per block: block b is tile b - tile_off[q] of query q = cand_tile_query(b), entries [lims[q] + 64 * tile, +64)
// of its list.  Lane l walks the chain of (q, rows[entry]); an entry that names no row gets NaN and walks nothing (the
// chain wants a row from every lane up to the last one that has one: the others pass row 0 and drop the result).  The
// score is written as a search reports it: through the order-preserving key, which folds -0 onto +0.
// n_scored[q] += the entries of the tile that were scored.
template <typename T, int METRIC>
__global__ __launch_bounds__(64) void cand_score_kernel(const T* __restrict__ corpus, uint32_t dim, uint32_t ld, const float* __restrict__ q,
                                                        const uint32_t* __restrict__ lims, const uint32_t* __restrict__ tile_off, uint32_t nq,
                                                        const uint32_t* __restrict__ rows, float* __restrict__ out,
                                                        uint32_t* __restrict__ n_scored) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* q_lds = smem;                       // [ld]
    float* tile = smem + ld;                   // [64][kTileStride]
    const uint32_t lane = threadIdx.x;
    const uint32_t qi = cand_tile_query(tile_off, nq, blockIdx.x);
    const uint64_t t = (uint64_t)lims[qi] + (uint64_t)(blockIdx.x - tile_off[qi]) * 64u + lane;
    const bool in = t < lims[qi + 1];
    const uint32_t row = in ? rows[t] : kCandNoRow;
    const bool valid = row != kCandNoRow;
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0ull) {                       // whole wave (single-wave block: no barrier is skipped)
        if (in) out[t] = __uint_as_float(kScoreNoneBits);
        return;
    }
    const float* qrow = q + (uint64_t)qi * ld;
    for (uint32_t i = lane; i < ld; i += 64) q_lds[i] = qrow[i];
    const float acc = canonical_chain_wave<T, METRIC>(corpus, dim, ld, q_lds, tile, valid ? row : 0u, 64 - __builtin_clzll(vmask));
    if (in) out[t] = valid && acc == acc ? key_to_score_rt(score_key_rt(acc, METRIC), METRIC) : __uint_as_float(kScoreNoneBits);
    if (lane == 0) atomicAdd(&n_scored[qi], (uint32_t)__builtin_popcountll(vmask));
}

void launch_cand_score(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q, const uint32_t* d_lims,
                       const uint32_t* d_tile_off, uint32_t nq, uint32_t n_tiles, const uint32_t* d_rows, float* d_out, uint32_t* d_n_scored,
                       hipStream_t s) {
    if (!nq || !n_tiles) return;
    const size_t lds = ((size_t)ld + 64 * kTileStride) * sizeof(float);
#define VROD_CK(TT, MM) \
    cand_score_kernel<TT, MM><<<n_tiles, 64, lds, s>>>((const TT*)d_corpus, dim, ld, d_q, d_lims, d_tile_off, nq, d_rows, d_out, d_n_scored)
    if (dtype == DT_BF16) { if (metric == M_COSINE) VROD_CK(bf16_t, M_COSINE); else VROD_CK(bf16_t, M_L2); }
    else { if (metric == M_COSINE) VROD_CK(float, M_COSINE); else VROD_CK(float, M_L2); }
#undef VROD_CK
}

}  // namespace vrod
