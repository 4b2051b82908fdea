// kernels_diverse.hip -- the greedy selection of a diversified search (vrod_search_diverse; gfx950).
//
// One launch after the first-stage search has left its certified [nq][pool] lists in device memory: one work-group per
// query picks min(k, m) of its m pool rows by exact greedy MMR (include/vrod.h):
//     step 0 takes position 0;  step t >= 1 takes the best  v_i = fl( fl(lambda * r_i) - fl(mu * pen_i) )
// over the positions not taken yet, pen_i = the best canonical score g(i, s) between pool row i and the rows s taken so
// far.  Everything a step needs stays in LDS: per position the local row, r, pen and a taken bit; the row taken last,
// widened to fp32; one chain tile per wave.  A step is
//     block arg-best over (v, position)      an order-preserving key per thread, wave reduction, then across the waves
//     the output slot                        one thread
//     the taken row into LDS                 16 B per thread along the stored row, bf16 widened as byid_gather_kernel does
//     g against that row, folded into pen    canonical_chain_wave (rescore_chain.h): a wave scores 64 positions per pass
// so only k * m chains ever run -- the m x m Gram matrix is never built.  Every loop is bounded by k, m (<= pool) or dim;
// there is no spin wait and no communication between work-groups.  mul_rn / sub_rn keep v's three roundings apart.
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "rescore_chain.h"
#include "diverse_plan.h"

namespace vrod {

// (v, position) as one key: larger = better.  score_key folds -0 onto +0 and puts NaN below every number (0; no number
// maps to 0); the low word makes the smaller position win a tie, an all-NaN step included.  0 = no position at all.
template <int METRIC>
__device__ __forceinline__ uint64_t diverse_key(float v, uint32_t pos) { return make_key(score_key<METRIC>(v), pos); }

__device__ __forceinline__ uint64_t diverse_wave_max(uint64_t key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(key >> 32), o), lo = __shfl_xor((uint32_t)key, o);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        key = other > key ? other : key;
    }
    return key;
}

// blockDim.x = 64 * waves (diverse_plan.h diverse_waves); dynamic LDS = diverse_lds_bytes(dim, pool, waves).
template <typename T, int METRIC>
__global__ __launch_bounds__(64 * kDiverseMaxWaves) void diverse_select_kernel(
    const T* __restrict__ corpus, uint32_t dim, uint32_t ld, const uint64_t* __restrict__ l_ids, const float* __restrict__ l_scores,
    uint32_t pool, uint32_t k, float lambda, float mu, uint64_t id_offset, uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
    float* __restrict__ out_mmr) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x, waves = nthreads >> 6;
    const uint32_t row_floats = diverse_row_floats(dim);
    float* sel_row = smem;                                              // [row_floats]
    float* tile = smem + row_floats + (size_t)wave * 64 * kTileStride;   // this wave's [64][kTileStride]
    // (the row and the tiles are whole multiples of 16 B: the 64-bit keys that follow them are aligned)
    uint64_t* s_best = reinterpret_cast<uint64_t*>(smem + row_floats + (size_t)waves * 64 * kTileStride);   // [kDiverseMaxWaves]
    uint32_t* s_taken = reinterpret_cast<uint32_t*>(s_best + kDiverseMaxWaves);   // [kDiverseMaxPool / 32]
    uint32_t* s_ctl = s_taken + kDiverseMaxPool / 32;                   // [0] = m, [1] = the position taken by this step
    uint32_t* s_idx = s_ctl + 4;                                        // [pool]
    float* s_r = reinterpret_cast<float*>(s_idx + pool);               // [pool]
    float* s_pen = s_r + pool;                                          // [pool]
    const uint32_t q = blockIdx.x;
    const uint64_t* li = l_ids + (uint64_t)q * pool;
    const float* ls = l_scores + (uint64_t)q * pool;
    uint64_t* oi = out_ids + (uint64_t)q * k;
    float* os = out_scores + (uint64_t)q * k;
    float* om = out_mmr ? out_mmr + (uint64_t)q * k : nullptr;

    // ---- the pool: filled slots are a prefix of the list; pen starts as NaN, which loses to the first number folded in
    if (tid == 0) s_ctl[0] = pool;
    if (tid < kDiverseMaxPool / 32) s_taken[tid] = 0u;
    __syncthreads();
    for (uint32_t p = tid; p < pool; p += nthreads) {
        const uint64_t id = li[p];
        const bool filled = id != ~0ull;
        s_idx[p] = filled ? (uint32_t)(id - id_offset) : 0u;
        s_r[p] = ls[p];
        s_pen[p] = __uint_as_float(kScoreNoneBits);
        if (!filled) atomicMin(&s_ctl[0], p);
    }
    __syncthreads();
    const uint32_t m = s_ctl[0];
    const uint32_t steps = k < m ? k : m;
    for (uint32_t j = steps + tid; j < k; j += nthreads) {   // the slots no step fills
        oi[j] = ~0ull;
        os[j] = __uint_as_float(kScoreNoneBits);
        if (om) om[j] = __uint_as_float(kScoreNoneBits);
    }

    for (uint32_t t = 0; t < steps; ++t) {
        // ---- arg-best over the positions not taken (step 0: position 0 as it is)
        uint64_t best = 0ull;
        if (t > 0) {
            for (uint32_t p = tid; p < m; p += nthreads) {
                if ((s_taken[p >> 5] >> (p & 31)) & 1u) continue;
                const float v = sub_rn(mul_rn(lambda, s_r[p]), mul_rn(mu, s_pen[p]));
                const uint64_t key = diverse_key<METRIC>(v, p);
                best = key > best ? key : best;
            }
            best = diverse_wave_max(best);
            if (lane == 0) s_best[wave] = best;
            __syncthreads();
        }
        if (tid == 0) {
            uint32_t sel = 0;
            float v = mul_rn(lambda, s_r[0]);
            if (t > 0) {
                for (uint32_t w = 0; w < waves; ++w) best = s_best[w] > best ? s_best[w] : best;
                sel = key_row(best);   // (t < m: a position is left, and every position's key is above 0)
                v = sub_rn(mul_rn(lambda, s_r[sel]), mul_rn(mu, s_pen[sel]));
            }
            s_ctl[1] = sel;
            s_taken[sel >> 5] |= 1u << (sel & 31);
            oi[t] = (uint64_t)s_idx[sel] + id_offset;
            os[t] = s_r[sel];
            if (om) om[t] = v;
        }
        if (t + 1 == steps) break;   // (uniform) nothing reads pen after the last step
        __syncthreads();
        const uint32_t sel = s_ctl[1];

        // ---- the taken row into LDS as fp32
        {
            constexpr uint32_t E = 16 / sizeof(T);   // elements per 16-B unit
            const u32x4* x = reinterpret_cast<const u32x4*>(corpus + (uint64_t)s_idx[sel] * ld);
            for (uint32_t u = tid; u * E < row_floats; u += nthreads) {   // (rows are whole 128-B lines: the unit lies inside the row)
                const u32x4 w = x[u];
                float* o = sel_row + u * E;
                if constexpr (sizeof(T) == 2) {
                    *reinterpret_cast<u32x4*>(o) = u32x4{w.x << 16, w.x & 0xFFFF0000u, w.y << 16, w.y & 0xFFFF0000u};
                    if (u * E + 4 < row_floats) *reinterpret_cast<u32x4*>(o + 4) = u32x4{w.z << 16, w.z & 0xFFFF0000u, w.w << 16, w.w & 0xFFFF0000u};
                } else {
                    *reinterpret_cast<u32x4*>(o) = w;
                }
            }
        }
        __syncthreads();

        // ---- g of every position not taken against that row, folded into pen.  The chain wants its rows as a prefix
        // of the wave: the taken positions of a chunk keep their lane and their result is dropped.
        for (uint32_t p0 = wave * 64; p0 < m; p0 += waves * 64) {
            const uint32_t p = p0 + lane;
            const bool open = p < m && !((s_taken[p >> 5] >> (p & 31)) & 1u);
            if (__ballot(open) == 0ull) continue;   // (wave-uniform; the chain has wave barriers only)
            const uint32_t nvalid = m - p0 < 64u ? m - p0 : 64u;
            const float g = canonical_chain_wave<T, METRIC>(corpus, dim, ld, sel_row, tile, p < m ? s_idx[p] : 0u, (int)nvalid);
            if (open && g == g) {   // a NaN g loses to any number; an equal g leaves pen as it is
                const float pen = s_pen[p];
                const bool better = METRIC == M_COSINE ? g > pen : g < pen;
                if (pen != pen || better) s_pen[p] = g;
            }
        }
        __syncthreads();   // pen is complete, and nobody reads the row any more
    }
}

void launch_diverse_select(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const uint64_t* d_list_ids,
                           const float* d_list_scores, uint32_t nq, uint32_t pool, uint32_t k, float lambda, uint64_t id_offset,
                           uint64_t* d_out_ids, float* d_out_scores, float* d_out_mmr, hipStream_t s) {
    if (!nq) return;
    const uint32_t waves = diverse_waves(dim, pool);
    const uint32_t lds = diverse_lds_bytes(dim, pool, waves);
    const float mu = 1.0f - lambda;   // fl(1 - lambda): one rounding, on the host
#define VROD_DV(TT, MM)                                                                                                            \
    do {                                                                                                                           \
        static bool attr_set = false;                                                                                              \
        if (!attr_set) {                                                                                                           \
            (void)hipFuncSetAttribute((const void*)diverse_select_kernel<TT, MM>, hipFuncAttributeMaxDynamicSharedMemorySize,      \
                                      (int)kDiverseLdsCap);                                                                        \
            attr_set = true;                                                                                                       \
        }                                                                                                                          \
        diverse_select_kernel<TT, MM><<<nq, 64 * waves, lds, s>>>((const TT*)d_corpus, dim, ld, d_list_ids, d_list_scores, pool, k, lambda, mu, \
                                                                  id_offset, d_out_ids, d_out_scores, d_out_mmr);                  \
    } while (0)
    if (dtype == DT_BF16) { if (metric == M_COSINE) VROD_DV(bf16_t, M_COSINE); else VROD_DV(bf16_t, M_L2); }
    else { if (metric == M_COSINE) VROD_DV(float, M_COSINE); else VROD_DV(float, M_L2); }
#undef VROD_DV
}

}  // namespace vrod
