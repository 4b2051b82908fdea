// dup_read.h -- how the device reads a stored row for duplicate-row detection and row lookup (kernels_dup.hip,
// kernels_rowfind.hip): the tombstone test, and the two load forms that DupPlan::read chooses between (dup_plan.h).
// Device code only.
#pragma once
#include "dup_plan.h"
#include "vrod_common.h"

namespace vrod {

__device__ __forceinline__ bool dup_row_dead(const uint32_t* __restrict__ del, uint64_t r) { return del && ((del[r >> 5] >> (r & 31u)) & 1u); }

// What one load of a row is: a 16-byte unit or a 32-bit word.  load(row base in bytes, j) is the row's j-th, terms() the
// hash terms of its words, differs() the comparison; `last`: the word path's final word, cut to the row's bits.
struct DupUnits {
    typedef u32x4_t T;
    static __device__ __forceinline__ T load(const unsigned char* __restrict__ row, uint32_t j) { return reinterpret_cast<const u32x4_t*>(row)[j]; }
    static __device__ __forceinline__ T cut(T v, bool, uint32_t) { return v; }
    static __device__ __forceinline__ uint64_t terms(T v, uint32_t j) {
        // dup_word_term of words 4j .. 4j + 3, the two keys stepped instead of multiplied
        uint32_t a = (4u * j + 1u) * kDupKeyA, b = (4u * j + 1u) * kDupKeyB;
        uint64_t s = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { s += (uint64_t)(uint32_t)(v[e] + a) * (uint64_t)(b | 1u); a += kDupKeyA; b += kDupKeyB; }
        return s;
    }
    static __device__ __forceinline__ bool differs(T x, T y) { return ((x[0] ^ y[0]) | (x[1] ^ y[1]) | (x[2] ^ y[2]) | (x[3] ^ y[3])) != 0u; }
};
struct DupWords {
    typedef uint32_t T;
    static __device__ __forceinline__ T load(const unsigned char* __restrict__ row, uint32_t j) { return reinterpret_cast<const uint32_t*>(row)[j]; }
    static __device__ __forceinline__ T cut(T v, bool last, uint32_t tail_mask) { return last ? v & tail_mask : v; }
    static __device__ __forceinline__ uint64_t terms(T v, uint32_t j) { return dup_word_term(v, j); }
    static __device__ __forceinline__ bool differs(T x, T y) { return x != y; }
};

}  // namespace vrod
