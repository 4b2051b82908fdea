// kernels_combine.hip -- a search by weighted examples (vrod_search_combined; gfx950).
//
// Two small launches around the ordinary search flow:
//   combine_queries_kernel  the [nq][dim] fp32 queries built on the device: per coordinate acc = +0, then for every operand
//                           in the caller's order acc = fl(acc + fl(w * x)) -- two roundings, never a fused multiply-add
//                           (mul_rn / add_rn of rescore_chain.h: under hipcc's default -ffp-contract=fast a plain
//                           product and sum, __fmul_rn / __fadd_rn included, are fused into v_pk_fma_f32).
//                           The operands are the query's prepared vector (if any) and its terms, prepared stored rows read
//                           as stored (bf16 widened).  The same launch checks every term id against the rows and the
//                           tombstones, every weight and every result for NaN / Inf, and raises one flag word;
//   drop_excluded_kernel    the search's [nq][k1] lists minus the query's excluded ids, cut to k.
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "rescore_chain.h"   // mul_rn / add_rn: one rounding each, out of the compiler's reach

namespace vrod {

__device__ inline bool combine_bit(const uint32_t* __restrict__ bits, uint64_t r) { return (bits[r >> 5] >> (r & 31)) & 1u; }
__device__ inline bool combine_finite(float f) { return __builtin_fabsf(f) <= 3.4028234663852886e38f; }

// ------------------------------------------------------------------ the combined queries
// `lanes` (64: a wave, 256: the work-group) lanes own query q and stride along the row in 16-B units of the STORED type,
// as byid_gather_kernel does: E = 4 fp32 or 8 bf16 coordinates per unit, rows are whole 128-B lines, so every unit that
// starts below dim lies inside the row (and inside the prepared vector's row of ld floats).  A lane keeps its unit's E
// accumulators in registers and walks the operands in order; the loads of four terms are issued ahead of the four steps
// that use them, the steps themselves stay in order.  A term id that is no live row contributes nothing and raises
// kCombineBadId; the search is not begun behind a raised flag, so what such a query holds is never used.
template <typename T>
__global__ __launch_bounds__(256) void combine_queries_kernel(const T* __restrict__ rows, uint32_t ld, uint32_t dim, uint64_t count,
                                                              uint64_t id_offset, const uint32_t* __restrict__ del,
                                                              const float* __restrict__ vec, const float* __restrict__ vec_w,
                                                              const uint32_t* __restrict__ term_lims, const uint64_t* __restrict__ term_ids,
                                                              const float* __restrict__ term_w, uint32_t nq, uint32_t lanes,
                                                              float* __restrict__ out, uint32_t* __restrict__ flag) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    constexpr uint32_t E = 16 / sizeof(T);   // elements per 16-B unit
    const uint32_t lane = threadIdx.x & (lanes - 1);
    const uint32_t q = blockIdx.x * (blockDim.x / lanes) + threadIdx.x / lanes;
    if (q >= nq) return;
    const uint32_t tb = term_lims[q], te = term_lims[q + 1];
    const float wv = vec ? (vec_w ? vec_w[q] : 1.0f) : 0.0f;
    uint32_t bad = combine_finite(wv) ? 0u : kCombineBadWeight;
    float* o = out + (uint64_t)q * dim;
    const bool vec_store = (dim & 3u) == 0;   // every query row then starts, and every group of four ends, on a 16-B boundary
    for (uint32_t u = lane; u * E < dim; u += lanes) {
        const uint32_t e0 = u * E;
        float acc[E];
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) acc[e] = 0.0f;
        if (vec) {
            const f32x4_t* x = reinterpret_cast<const f32x4_t*>(vec + (uint64_t)q * ld + e0);
#pragma unroll
            for (uint32_t g = 0; g < E; g += 4) {
                const f32x4_t v = x[g >> 2];
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) acc[g + e] = add_rn(acc[g + e], mul_rn(wv, v[e]));
            }
        }
        for (uint32_t t0 = tb; t0 < te; t0 += 4) {
            u32x4_t v[4];
            float w[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                v[i] = u32x4_t{0u, 0u, 0u, 0u};
                w[i] = 0.0f;
                if (t0 + i < te) {
                    const uint64_t id = term_ids[t0 + i];
                    const uint64_t row = id - id_offset;
                    bool ok = id >= id_offset && row < count;
                    if (ok && del) ok = !combine_bit(del, row);
                    w[i] = term_w[t0 + i];
                    if (!ok) bad |= kCombineBadId;
                    if (!combine_finite(w[i])) bad |= kCombineBadWeight;
                    if (ok) v[i] = reinterpret_cast<const u32x4_t*>(rows + row * (uint64_t)ld)[u];
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                if (t0 + i < te) {   // (a step that is not there must not run: -0 + fl(w * 0) is +0)
                    float f[E];
                    if constexpr (sizeof(T) == 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) { f[2 * e] = __uint_as_float(v[i][e] << 16); f[2 * e + 1] = __uint_as_float(v[i][e] & 0xFFFF0000u); }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(v[i][e]);
                    }
#pragma unroll
                    for (uint32_t e = 0; e < E; ++e) acc[e] = add_rn(acc[e], mul_rn(w[i], f[e]));
                }
            }
        }
#pragma unroll
        for (uint32_t e = 0; e < E; ++e)
            if (e0 + e < dim && !combine_finite(acc[e])) bad |= kCombineNonFinite;
        if (vec_store && e0 + E <= dim) {
#pragma unroll
            for (uint32_t g = 0; g < E; g += 4) {
                const f32x4_t r = {acc[g], acc[g + 1], acc[g + 2], acc[g + 3]};
                *reinterpret_cast<f32x4_t*>(o + e0 + g) = r;
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < E; ++e)
                if (e0 + e < dim) o[e0 + e] = acc[e];
        }
    }
    if (bad) atomicOr(flag, bad);
}

// ------------------------------------------------------------------ drop by id set
// One work-group per query.  Its excluded ids -- the exclude list, then (with_terms) its term ids: at most
// kCombineMaxExclude in all, which the host has checked -- go into LDS.  The list is walked in chunks of 256 positions:
// each lane tests its entry against the set, survivors are compacted in order (ballot ranks within a wave, the waves'
// totals through LDS, as byid_live_kernel), the first k are written and the rest of the row is padded unfilled.  An
// unfilled list entry survives as it is: VROD_ID_NONE in the set excludes nothing.
__global__ __launch_bounds__(256) void drop_excluded_kernel(const uint64_t* __restrict__ l_ids, const float* __restrict__ l_scores, uint32_t k1,
                                                            const uint32_t* __restrict__ excl_lims, const uint64_t* __restrict__ excl_ids,
                                                            const uint32_t* __restrict__ term_lims, const uint64_t* __restrict__ term_ids,
                                                            uint32_t k, uint64_t* __restrict__ out_ids, float* __restrict__ out_scores) {
    __shared__ uint64_t s_set[kCombineMaxExclude];
    __shared__ uint32_t s_wave[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t xb = excl_lims ? excl_lims[q] : 0u, nx = excl_lims ? excl_lims[q + 1] - xb : 0u;
    const uint32_t tb = term_lims ? term_lims[q] : 0u, nt = term_lims ? term_lims[q + 1] - tb : 0u;
    const uint32_t n_set = min(nx + nt, kCombineMaxExclude);
    for (uint32_t i = tid; i < n_set; i += 256) s_set[i] = i < nx ? excl_ids[xb + i] : term_ids[tb + (i - nx)];
    __syncthreads();
    const uint64_t* li = l_ids + (uint64_t)q * k1;
    const float* ls = l_scores + (uint64_t)q * k1;
    uint64_t* oi = out_ids + (uint64_t)q * k;
    float* os = out_scores + (uint64_t)q * k;
    uint32_t base = 0;   // survivors so far (the same in every lane: the loop's exit is uniform)
    for (uint32_t p0 = 0; p0 < k1 && base < k; p0 += 256) {
        const uint32_t p = p0 + tid;
        uint64_t id = ~0ull;
        float sc = __uint_as_float(kScoreNoneBits);
        bool keep = p < k1;
        if (keep) {
            id = li[p];
            sc = ls[p];
            if (id != ~0ull)
                for (uint32_t i = 0; i < n_set; ++i) keep &= s_set[i] != id;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = base;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        const uint32_t j = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (keep && j < k) { oi[j] = id; os[j] = sc; }
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    for (uint32_t j = base + tid; j < k; j += 256) { oi[j] = ~0ull; os[j] = __uint_as_float(kScoreNoneBits); }
}

// ------------------------------------------------------------------ launchers
void launch_combine_queries(const void* d_corpus, int dtype, uint32_t ld, uint32_t dim, uint64_t count, uint64_t id_offset, const uint32_t* d_del,
                            const float* d_vec, const float* d_vec_w, const uint32_t* d_term_lims, const uint64_t* d_term_ids,
                            const float* d_term_w, uint32_t nq, float* d_out, uint32_t* d_flag, hipStream_t s) {
    if (!nq) return;
    const uint32_t lanes = combine_lanes_per_query(dim, dtype == DT_BF16 ? 2u : 4u);
    const unsigned g = (nq + 256 / lanes - 1) / (256 / lanes);
    if (dtype == DT_BF16)
        combine_queries_kernel<bf16_t><<<g, 256, 0, s>>>((const bf16_t*)d_corpus, ld, dim, count, id_offset, d_del, d_vec, d_vec_w, d_term_lims,
                                                         d_term_ids, d_term_w, nq, lanes, d_out, d_flag);
    else
        combine_queries_kernel<float><<<g, 256, 0, s>>>((const float*)d_corpus, ld, dim, count, id_offset, d_del, d_vec, d_vec_w, d_term_lims,
                                                        d_term_ids, d_term_w, nq, lanes, d_out, d_flag);
}

void launch_drop_excluded(const uint64_t* d_list_ids, const float* d_list_scores, uint32_t k1, const uint32_t* d_excl_lims,
                          const uint64_t* d_excl_ids, const uint32_t* d_term_lims, const uint64_t* d_term_ids, uint32_t nq, uint32_t k,
                          uint64_t* d_out_ids, float* d_out_scores, hipStream_t s) {
    if (!nq) return;
    drop_excluded_kernel<<<nq, 256, 0, s>>>(d_list_ids, d_list_scores, k1, d_excl_lims, d_excl_ids, d_term_lims, d_term_ids, k, d_out_ids,
                                            d_out_scores);
}

}  // namespace vrod
