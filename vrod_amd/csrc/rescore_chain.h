// rescore_chain.h -- the canonical (oracle-order) chain of one wave: 64 (query, row) chains, one per lane.
// Shared by the candidate re-score (kernels_rescore.hip) and the range search's re-score-and-cut (kernels_range.hip):
// there is ONE spelling of the chain   acc = acc + (q[j] * x[j])   in the library's candidate form.
#pragma once
#include "vrod_common.h"

namespace vrod {

__device__ __forceinline__ float mul_rn(float a, float b) {
    float r;
    asm("v_mul_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float add_rn(float a, float b) {
    float r;
    asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
    float r;
    asm("v_sub_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

constexpr int kTileStride = 68;  // dwords: 16-B aligned rows, conflict-free b128 column walk

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The chains of one wave over one query: lane l walks row my_row of the corpus against q_lds [ld] (the prepared query,
// in LDS), staged through the wave-private `tile` [64][kTileStride].  The lanes with a row are a prefix of the wave,
// `nvalid` of them (>= 1); the others pass any valid row (0) and ignore the result.
// Each 64-element chunk of the 64 rows is fetched with 16-B loads, all issued before the
// first LDS write (the chain itself is sequential, the loads must not be), and then every
// lane walks its own row of the tile in order.
template <typename T, int METRIC>
__device__ __forceinline__ float canonical_chain_wave(const T* __restrict__ corpus, uint32_t dim, uint32_t ld, const float* q_lds,
                                                      float* tile, uint32_t my_row, int nvalid) {
    constexpr int EPU = 16 / (int)sizeof(T);   // elements per 16-B load: 4 fp32 / 8 bf16
    constexpr int LPC = 64 / EPU;              // lanes covering one row's 64-element chunk
    constexpr int RPI = 64 / LPC;              // rows per load instruction
    constexpr int NI = 64 / RPI;               // load instructions per chunk
    const int lane = threadIdx.x & 63;
    // valid slots are a prefix of the wave; rows beyond it are not fetched
    const int ni_used = (nvalid + RPI - 1) / RPI;
    const int sub = lane / LPC, part = lane % LPC;

    float acc = 0.0f;
    // The chain is sequential and latency-bound; the row gathers must not be: the loads of chunks
    // c+1 .. c+D-1 are in flight while the chain of chunk c runs (ring of D register sets; with
    // one chunk ahead a 768-d re-score waited a full gather latency twelve times: 38-44 us).
    constexpr int D = 3;
    u32x4 v[D][NI];
    auto fetch = [&](u32x4 (&vs)[NI], uint32_t j0) {
        const uint32_t e0 = j0 + part * EPU;  // first element this lane fetches
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            vs[it] = u32x4{0u, 0u, 0u, 0u};
            if (it < ni_used) {
                const uint32_t row = __shfl(my_row, it * RPI + sub);
                if (e0 < ld) vs[it] = *reinterpret_cast<const u32x4*>(corpus + (uint64_t)row * ld + e0);
            }
        }
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if ((uint32_t)d * 64 < dim) fetch(v[d], d * 64);
    for (uint32_t jb = 0; jb < dim; jb += 64 * D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const uint32_t j0 = jb + d * 64;
            if (j0 >= dim) break;
#pragma unroll
            for (int it = 0; it < NI; ++it) {
                float* t = tile + (it * RPI + sub) * kTileStride + part * EPU;
                if constexpr (sizeof(T) == 4) {
                    *reinterpret_cast<u32x4*>(t) = v[d][it];
                } else {
                    *reinterpret_cast<u32x4*>(t) = u32x4{v[d][it].x << 16, v[d][it].x & 0xFFFF0000u, v[d][it].y << 16, v[d][it].y & 0xFFFF0000u};
                    *reinterpret_cast<u32x4*>(t + 4) = u32x4{v[d][it].z << 16, v[d][it].z & 0xFFFF0000u, v[d][it].w << 16, v[d][it].w & 0xFFFF0000u};
                }
            }
            if (j0 + 64 * D < dim) fetch(v[d], j0 + 64 * D);
            // the tile (and q_lds on the first pass) is wave-private: in-order LDS + a compiler fence
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t jn = dim - j0 < 64 ? dim - j0 : 64;
            const float* trow = tile + lane * kTileStride;
            if (jn == 64) {
                // whole chunk: fully unrolled, so the LDS reads and the products (independent)
                // run ahead of the one thing that is serial, the 64 dependent adds
#pragma unroll
                for (uint32_t l = 0; l < 64; l += 4) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(trow + l);
                    const f32x4 qq = *reinterpret_cast<const f32x4*>(q_lds + j0 + l);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (METRIC == M_COSINE) {
                            acc = add_rn(acc, mul_rn(qq[e], x[e]));
                        } else {
                            const float dd = sub_rn(qq[e], x[e]);
                            acc = add_rn(acc, mul_rn(dd, dd));
                        }
                    }
                }
            } else {
                for (uint32_t l = 0; l < jn; l += 4) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(trow + l);
                    const f32x4 qq = *reinterpret_cast<const f32x4*>(q_lds + j0 + l);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (l + e < jn) {
                            if constexpr (METRIC == M_COSINE) {
                                acc = add_rn(acc, mul_rn(qq[e], x[e]));
                            } else {
                                const float dd = sub_rn(qq[e], x[e]);
                                acc = add_rn(acc, mul_rn(dd, dd));
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    return acc;
}

}  // namespace vrod
