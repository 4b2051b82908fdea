// kernels_snapshot.hip -- the device side of vrod_index_save / vrod_index_load (gfx950).
//
// A snapshot stores the rows dense, [count][dim] elements, whatever the handle's row pitch is, and every section carries
// a checksum that is a SUM over its u32 words (snapshot_plan.h).  Three kernels:
//   pack      rows at pitch ld -> a dense staging buffer, and the checksum of what it wrote, in the same pass (save);
//   unpack    a dense staging buffer as it arrived over PCIe -> rows at pitch ld, and the checksum of what it read (load).
//             It writes the row's elements only: the padding up to ld is zero already, index_reserve clears every
//             allocation it makes;
//   checksum  a plain byte range (the side arrays, vrod_snapshot_checksum_device).
// All three are streaming passes with no reuse: a flat grid-stride loop, 16-byte accesses wherever a dense row is a whole
// number of 16-byte units (dim * element size % 16 == 0: every width the scans are tuned for), u32 words otherwise.  A
// bf16 row of odd dim makes dense words straddle two rows: the word path addresses each of a word's two elements on its
// own.  The sum is accumulated per thread in u64, reduced over the wave by shuffles, over the block through LDS, and one
// 64-bit atomic add per block goes to the device word: any grid and any chunking give the same 64 bits.
// A chunk is at most kSnapChunkBytesMax (snapshot_plan.h) of dense bytes, so chunk-local word and unit indices fit 32 bits.
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "snapshot_plan.h"

namespace vrod {

__device__ inline uint64_t snap_mix_dev(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the terms of the four words of one 16-byte unit whose first word has the global index i
__device__ inline uint64_t snap_unit_terms(u32x4_t v, uint64_t i) {
    uint64_t g = (i + 1) * kSnapGolden, s = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { s += snap_mix_dev((uint64_t)v[e] + g); g += kSnapGolden; }
    return s;
}
__device__ inline uint64_t snap_word_term_dev(uint32_t w, uint64_t i) { return snap_mix_dev((uint64_t)w + (i + 1) * kSnapGolden); }

// every thread's partial sum -> one atomic add per block (256 threads)
__device__ inline void snap_block_add(uint64_t s, unsigned long long* __restrict__ sum) {
    __shared__ uint64_t part[4];
    for (int o = 32; o > 0; o >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t t = part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd(sum, (unsigned long long)t);
    }
}

// ------------------------------------------------------------------ 16-byte path: upr units per dense row, ldu per stored row
// PACK: stored -> dense; else dense -> stored.  n_units = rows * upr < 2^32.
template <bool PACK>
__global__ __launch_bounds__(256) void snap_rows_units_kernel(const u32x4_t* __restrict__ src, u32x4_t* __restrict__ dst, uint32_t n_units,
                                                              uint32_t upr, uint32_t ldu, uint64_t first_word,
                                                              unsigned long long* __restrict__ sum) {
    uint64_t s = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u < n_units; u += stride) {
        const uint32_t row = u / upr, c = u - row * upr;
        const uint64_t stored = (uint64_t)row * ldu + c;
        const u32x4_t v = src[PACK ? stored : (uint64_t)u];
        dst[PACK ? (uint64_t)u : stored] = v;
        s += snap_unit_terms(v, first_word + (uint64_t)u * 4);
    }
    snap_block_add(s, sum);
}

// ------------------------------------------------------------------ word path
// element e (< n_elems) of the chunk's dense payload lives at stored element (e / dim) * ld + e % dim
template <typename T>
__global__ __launch_bounds__(256) void snap_pack_words_kernel(const T* __restrict__ rows, uint32_t* __restrict__ dense, uint32_t n_words,
                                                              uint64_t n_elems, uint32_t dim, uint32_t ld, uint64_t first_word,
                                                              unsigned long long* __restrict__ sum) {
    uint64_t s = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_words; j += stride) {
        uint32_t w;
        if constexpr (sizeof(T) == 4) {
            const uint32_t row = j / dim, c = j - row * dim;
            w = rows[(uint64_t)row * ld + c];
        } else {
            const uint64_t e0 = (uint64_t)j * 2;
            const uint32_t row = (uint32_t)(e0 / dim), c = (uint32_t)(e0 - (uint64_t)row * dim);
            const uint32_t lo = rows[(uint64_t)row * ld + c];
            uint32_t hi = 0;   // the zero fill of a payload that ends on half a word
            if (e0 + 1 < n_elems) hi = c + 1 < dim ? rows[(uint64_t)row * ld + c + 1] : rows[(uint64_t)(row + 1) * ld];
            w = lo | (hi << 16);
        }
        dense[j] = w;
        s += snap_word_term_dev(w, first_word + j);
    }
    snap_block_add(s, sum);
}

template <typename T>
__global__ __launch_bounds__(256) void snap_unpack_words_kernel(const uint32_t* __restrict__ dense, T* __restrict__ rows, uint32_t n_words,
                                                                uint64_t n_elems, uint32_t dim, uint32_t ld, uint64_t first_word,
                                                                unsigned long long* __restrict__ sum) {
    uint64_t s = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_words; j += stride) {
        const uint32_t w = dense[j];
        s += snap_word_term_dev(w, first_word + j);
        if constexpr (sizeof(T) == 4) {
            const uint32_t row = j / dim, c = j - row * dim;
            rows[(uint64_t)row * ld + c] = w;
        } else {
            const uint64_t e0 = (uint64_t)j * 2;
            const uint32_t row = (uint32_t)(e0 / dim), c = (uint32_t)(e0 - (uint64_t)row * dim);
            rows[(uint64_t)row * ld + c] = (T)(w & 0xFFFFu);
            if (e0 + 1 < n_elems) {   // (the other half of the payload's last word is fill, not a row's element)
                if (c + 1 < dim) rows[(uint64_t)row * ld + c + 1] = (T)(w >> 16);
                else rows[(uint64_t)(row + 1) * ld] = (T)(w >> 16);
            }
        }
    }
    snap_block_add(s, sum);
}

// ------------------------------------------------------------------ plain range: n_bytes at a 4-byte aligned address
// VEC: the address is 16-byte aligned, whole units first.  The words behind them, and the zero-filled last one, singly.
template <bool VEC>
__global__ __launch_bounds__(256) void snap_checksum_kernel(const unsigned char* __restrict__ bytes, uint64_t n_bytes, uint64_t first_word,
                                                            unsigned long long* __restrict__ sum) {
    uint64_t s = 0;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_full = n_bytes / 4, n_units = VEC ? n_full / 4 : 0;
    if constexpr (VEC) {
        const u32x4_t* x = reinterpret_cast<const u32x4_t*>(bytes);
        for (uint64_t u = tid; u < n_units; u += stride) s += snap_unit_terms(x[u], first_word + u * 4);
    }
    const uint32_t* wds = reinterpret_cast<const uint32_t*>(bytes);
    for (uint64_t j = n_units * 4 + tid; j < n_full; j += stride) s += snap_word_term_dev(wds[j], first_word + j);
    if (tid == 0 && n_bytes % 4) {
        uint32_t w = 0;
        for (uint32_t b = 0; b < n_bytes % 4; ++b) w |= (uint32_t)bytes[n_full * 4 + b] << (8 * b);
        s += snap_word_term_dev(w, first_word + n_full);
    }
    snap_block_add(s, sum);
}

// ------------------------------------------------------------------ launchers
// streaming passes: at most 2048 work-groups of 256, the rest by the grid-stride loops
static inline unsigned snap_grid(uint64_t items) { return (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(1, (items + 255) / 256)); }

static void launch_snap_rows(bool pack, const void* d_src, void* d_dst, uint64_t n_rows, uint32_t dim, uint32_t ld, int dtype,
                             uint64_t first_word, uint64_t* d_sum, hipStream_t s) {
    if (!n_rows) return;
    const uint32_t es = dtype == DT_BF16 ? 2 : 4;
    const uint64_t dense_bytes = n_rows * dim * es;
    unsigned long long* sum = (unsigned long long*)d_sum;
    if ((uint64_t)dim * es % 16 == 0) {
        const uint32_t upr = dim * es / 16, ldu = ld * es / 16, n_units = (uint32_t)(dense_bytes / 16);
        if (pack) snap_rows_units_kernel<true><<<snap_grid(n_units), 256, 0, s>>>((const u32x4_t*)d_src, (u32x4_t*)d_dst, n_units, upr, ldu, first_word, sum);
        else snap_rows_units_kernel<false><<<snap_grid(n_units), 256, 0, s>>>((const u32x4_t*)d_src, (u32x4_t*)d_dst, n_units, upr, ldu, first_word, sum);
        return;
    }
    const uint32_t n_words = (uint32_t)((dense_bytes + 3) / 4);
    const uint64_t n_elems = n_rows * dim;
    const unsigned grid = snap_grid(n_words);
    if (dtype == DT_BF16) {
        if (pack) snap_pack_words_kernel<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)d_src, (uint32_t*)d_dst, n_words, n_elems, dim, ld, first_word, sum);
        else snap_unpack_words_kernel<bf16_t><<<grid, 256, 0, s>>>((const uint32_t*)d_src, (bf16_t*)d_dst, n_words, n_elems, dim, ld, first_word, sum);
    } else {
        if (pack) snap_pack_words_kernel<uint32_t><<<grid, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_dst, n_words, n_elems, dim, ld, first_word, sum);
        else snap_unpack_words_kernel<uint32_t><<<grid, 256, 0, s>>>((const uint32_t*)d_src, (uint32_t*)d_dst, n_words, n_elems, dim, ld, first_word, sum);
    }
}

void launch_snapshot_pack(const void* d_rows, uint64_t n_rows, uint32_t dim, uint32_t ld, int dtype, void* d_dense, uint64_t first_word,
                          uint64_t* d_sum, hipStream_t s) {
    launch_snap_rows(true, d_rows, d_dense, n_rows, dim, ld, dtype, first_word, d_sum, s);
}

void launch_snapshot_unpack(const void* d_dense, uint64_t n_rows, uint32_t dim, uint32_t ld, int dtype, void* d_rows, uint64_t first_word,
                            uint64_t* d_sum, hipStream_t s) {
    launch_snap_rows(false, d_dense, d_rows, n_rows, dim, ld, dtype, first_word, d_sum, s);
}

void launch_snapshot_checksum(const void* d_bytes, uint64_t n_bytes, uint64_t first_word, uint64_t* d_sum, hipStream_t s) {
    if (!n_bytes) return;
    const unsigned char* p = (const unsigned char*)d_bytes;
    unsigned long long* sum = (unsigned long long*)d_sum;
    if ((uintptr_t)p % 16 == 0) snap_checksum_kernel<true><<<snap_grid(n_bytes / 16 + 1), 256, 0, s>>>(p, n_bytes, first_word, sum);
    else snap_checksum_kernel<false><<<snap_grid(n_bytes / 4 + 1), 256, 0, s>>>(p, n_bytes, first_word, sum);
}

}  // namespace vrod
