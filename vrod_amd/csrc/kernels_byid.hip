// kernels_byid.hip -- searches whose queries are stored rows (vrod_search_by_ids, vrod_knn_graph; gfx950).
//
// Three small launches around the ordinary search flow:
//   byid_live_kernel    a batch of the graph's id range with deleted rows in it: the live rows, compacted, and for
//                       every row of the range its place among them (deleted rows never reach the scan);
//   byid_gather_kernel  the prepared rows named by ids (or by a row range) copied out of the corpus as [nq][dim] fp32
//                       queries -- bf16 widened, fp32 copied, nothing normalised or rounded: the search that follows
//                       takes them as given -- with the range / tombstone check of every id folded in;
//   byid_drop_self_kernel  the search's [nq][k + 1] lists minus the entry that carries the query's own id, cut to k.
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

__device__ inline bool byid_bit(const uint32_t* __restrict__ bits, uint64_t r) { return (bits[r >> 5] >> (r & 31)) & 1u; }

// ------------------------------------------------------------------ live rows of a range
// ONE work-group walks rows [row0, row0 + m) in steps of 256: ballot ranks within a wave, the waves' totals through LDS.
// d_live[j] = the j-th live row (ascending), d_src[i] = j for the live row row0 + i, ~0u for a deleted one.
__global__ __launch_bounds__(256) void byid_live_kernel(const uint32_t* __restrict__ del, uint64_t row0, uint32_t m,
                                                        uint32_t* __restrict__ d_live, uint32_t* __restrict__ d_src) {
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < m; i0 += 256) {
        const uint32_t i = i0 + tid;
        const bool live = i < m && !byid_bit(del, row0 + i);
        const unsigned long long bal = __ballot(live);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = base;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        const uint32_t j = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (i < m) d_src[i] = live ? j : ~0u;
        if (live) d_live[j] = (uint32_t)(row0 + i);
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
}

// ------------------------------------------------------------------ query gather
// One wave per query, 16 B per lane along the stored row (rows are whole 128-B lines: every 16-B unit that starts below
// dim lies inside the row).  Query q is row d_ids[q] - id_offset (checked: a current row that is not deleted, else the
// flag is raised and the query is a zero row), or row d_rows[q], or row base_row + q (both checked against the count).
// bad_flag may be null (the host has checked already): a bad query is then a zero row and nothing else.
template <typename T>
__global__ __launch_bounds__(256) void byid_gather_kernel(const T* __restrict__ rows, uint32_t ld, uint32_t dim, uint64_t count,
                                                          uint64_t id_offset, const uint32_t* __restrict__ del,
                                                          const uint64_t* __restrict__ d_ids, const uint32_t* __restrict__ d_rows,
                                                          uint64_t base_row, uint32_t nq, float* __restrict__ out,
                                                          uint32_t* __restrict__ bad_flag) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    constexpr uint32_t E = 16 / sizeof(T);   // elements per 16-B unit
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;
    uint64_t row;
    bool ok;
    if (d_ids) {
        const uint64_t id = d_ids[q];
        row = id - id_offset;
        ok = id >= id_offset && row < count;
        if (ok && del) ok = !byid_bit(del, row);
    } else {
        row = d_rows ? (uint64_t)d_rows[q] : base_row + q;
        ok = row < count;
    }
    if (!ok && lane == 0 && bad_flag) atomicOr(bad_flag, 1u);
    const u32x4_t* x = reinterpret_cast<const u32x4_t*>(rows + (ok ? row : 0) * (uint64_t)ld);
    float* o = out + (uint64_t)q * dim;
    const bool vec = (dim & 3u) == 0;   // every query row then starts, and every group of four ends, on a 16-B boundary
    for (uint32_t u = lane; u * E < dim; u += 64) {
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (ok) v = x[u];
        float f[E];
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { f[2 * e] = __uint_as_float(v[e] << 16); f[2 * e + 1] = __uint_as_float(v[e] & 0xFFFF0000u); }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(v[e]);
        }
        const uint32_t e0 = u * E;
        if (vec && e0 + E <= dim) {
#pragma unroll
            for (uint32_t g = 0; g < E; g += 4) {
                const f32x4_t w = {f[g], f[g + 1], f[g + 2], f[g + 3]};
                *reinterpret_cast<f32x4_t*>(o + e0 + g) = w;
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < E; ++e)
                if (e0 + e < dim) o[e0 + e] = f[e];
        }
    }
}

// ------------------------------------------------------------------ self drop
// One wave per output row i.  Its list is row d_src[i] of the search's results (i itself when d_src is null; ~0u: the
// row gets no list -- a deleted row of the graph's range -- and is written unfilled), its own id d_self[i] (base_id + i
// when d_self is null).  A ballot finds the one position that carries the id, if any; the k entries around it are
// copied in order.  k1 > k: position k of the list exists.
__global__ __launch_bounds__(256) void byid_drop_self_kernel(const uint64_t* __restrict__ l_ids, const float* __restrict__ l_scores,
                                                             uint32_t k1, const uint32_t* __restrict__ d_src,
                                                             const uint64_t* __restrict__ d_self, uint64_t base_id, uint32_t n_out,
                                                             uint32_t k, uint64_t* __restrict__ out_ids, float* __restrict__ out_scores) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n_out) return;
    uint64_t* oi = out_ids + (uint64_t)i * k;
    float* os = out_scores + (uint64_t)i * k;
    const uint32_t src = d_src ? d_src[i] : i;
    if (src == ~0u) {
        for (uint32_t j = lane; j < k; j += 64) { oi[j] = ~0ull; os[j] = __uint_as_float(kScoreNoneBits); }
        return;
    }
    const uint64_t self = d_self ? d_self[i] : base_id + i;
    const uint64_t* li = l_ids + (uint64_t)src * k1;
    const float* ls = l_scores + (uint64_t)src * k1;
    uint32_t pos = k1;   // (every value below is the same in all lanes: the loop's exit is uniform)
    for (uint32_t p0 = 0; p0 < k1; p0 += 64) {
        const uint32_t p = p0 + lane;
        const unsigned long long hit = __ballot(p < k1 && li[p] == self);
        if (hit) { pos = p0 + (uint32_t)__ffsll((long long)hit) - 1u; break; }
    }
    for (uint32_t j = lane; j < k; j += 64) {
        const uint32_t s = j < pos ? j : j + 1;
        const bool in = s < k1;
        oi[j] = in ? li[s] : ~0ull;
        os[j] = in ? ls[s] : __uint_as_float(kScoreNoneBits);
    }
}

// ------------------------------------------------------------------ launchers
void launch_byid_live(const uint32_t* d_del, uint64_t row0, uint32_t m, uint32_t* d_live, uint32_t* d_src, hipStream_t s) {
    if (!m) return;
    byid_live_kernel<<<1, 256, 0, s>>>(d_del, row0, m, d_live, d_src);
}

void launch_byid_gather(const void* d_corpus, int dtype, uint32_t ld, uint32_t dim, uint64_t count, uint64_t id_offset,
                        const uint32_t* d_del, const uint64_t* d_ids, const uint32_t* d_rows, uint64_t base_row, uint32_t nq, float* d_out,
                        uint32_t* d_bad_flag, hipStream_t s) {
    if (!nq) return;
    const unsigned g = (nq + 3) / 4;
    if (dtype == DT_BF16)
        byid_gather_kernel<bf16_t><<<g, 256, 0, s>>>((const bf16_t*)d_corpus, ld, dim, count, id_offset, d_del, d_ids, d_rows, base_row, nq,
                                                     d_out, d_bad_flag);
    else
        byid_gather_kernel<float><<<g, 256, 0, s>>>((const float*)d_corpus, ld, dim, count, id_offset, d_del, d_ids, d_rows, base_row, nq,
                                                    d_out, d_bad_flag);
}

void launch_byid_drop_self(const uint64_t* d_list_ids, const float* d_list_scores, uint32_t k1, const uint32_t* d_src, const uint64_t* d_self,
                           uint64_t base_id, uint32_t n_out, uint32_t k, uint64_t* d_out_ids, float* d_out_scores, hipStream_t s) {
    if (!n_out) return;
    byid_drop_self_kernel<<<(n_out + 3) / 4, 256, 0, s>>>(d_list_ids, d_list_scores, k1, d_src, d_self, base_id, n_out, k, d_out_ids,
                                                         d_out_scores);
}

}  // namespace vrod
