// prep_chain.h -- the arithmetic of row and query preparation, in one place (device code).  kernels_ingest.hip (the
// prepare of every row that reaches a handle, from host or device memory) and kernels_prep.hip (the query prepare)
// include it, so that a query meets rows prepared by the chain and the divide that prepared it.
//
// Spec (DESIGN.md "Scan spec", oracle/vrod_oracle.c orc_prepare_row): COSINE: x / sqrt(sum x^2), the sum accumulated
// left to right in fp64 (v * v is exact in fp64 for an fp32 v, so fma(v, v, ss) == ss + v*v rounded once), the divide
// in fp64, then rounded to fp32; zero rows stay zero.  BF16: round to nearest even, after the normalisation.
#pragma once
#include "vrod_common.h"

namespace vrod {

// NaN or Inf
__device__ inline bool prep_is_bad(float f) { return !(__builtin_fabsf(f) <= 3.4028234663852886e38f); }

// one step of the norm chain
__device__ inline double prep_chain_step(float f, double ss) {
    const double v = (double)f;
    return __builtin_fma(v, v, ss);
}

// The chain over a 16-B aligned row in LDS, walked by ONE thread: the same left-to-right chain, fed by 16-B LDS reads
// issued ahead of it (one scalar LDS read per step left the chain waiting ~100 cycles per element: 23 us at d = 768).
__device__ inline double prep_chain_lds(const float* row, uint32_t dim) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    double ss = 0.0;
    uint32_t j = 0;
#pragma unroll 4
    for (; j + 8 <= dim; j += 8) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(row + j);
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(row + j + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = prep_chain_step(a[e], ss);
#pragma unroll
        for (int e = 0; e < 4; ++e) ss = prep_chain_step(b[e], ss);
    }
    for (; j < dim; ++j) ss = prep_chain_step(row[j], ss);
    return ss;
}

// v / nrm in fp64, rounded to fp32; a zero row stays zero
__device__ inline float prep_scale(float v, double nrm) { return nrm == 0.0 ? 0.0f : (float)((double)v / nrm); }

}  // namespace vrod
