// kernels_mutate.hip -- the corpus mutations behind vrod_index_update and vrod_index_compact (gfx950).
//
// They stand behind the reference's UPDATE (src/command/types.rs:82, builder.rs:53) and REINDEX
// (types.rs:134, builder.rs:73) commands.  Both are HBM-bound row moves: one wave per row, 16 B per lane
// (rows are whole 128-B lines), a grid-stride loop over the rows.  Neither touches a scan kernel.
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

// ------------------------------------------------------------------ update: scatter prepared rows
// staged[i] (prepared by launch_ingest_rows) becomes corpus row dst[i]; dst[i] == kScatterSkip leaves row i out (an
// id named again later in the same call: the last occurrence wins, and two waves never write one row).  Also the
// row's fast squared norm -- the bits row_fastnorm_kernel gives the same row (vrod_common.h fastnorm_fold) -- folded
// into the handle's maximum, and on an fp32 handle whose bf16 planes exist the [hi | lo] planes of the row, element
// by element what split_rows_kernel<0> writes.
template <typename T>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const T* __restrict__ staged, const uint32_t* __restrict__ dst,
                                                           uint64_t n, uint32_t ld, T* __restrict__ corpus,
                                                           float* __restrict__ xn2, uint32_t* __restrict__ max_bits,
                                                           bf16_t* __restrict__ planes, uint64_t planes_rows, uint32_t ldp) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t units = ld * (uint32_t)sizeof(T) / 16;
    float wave_max = 0.0f;
    for (uint64_t r = wave; r < n; r += nwaves) {
        const uint32_t d = dst[r];   // the same for the whole wave
        if (d == kScatterSkip) continue;
        const T* src = staged + r * (uint64_t)ld;
        const u32x4_t* x = reinterpret_cast<const u32x4_t*>(src);
        u32x4_t* o = reinterpret_cast<u32x4_t*>(corpus + (uint64_t)d * ld);
        float s = 0.0f;
        for (uint32_t j = lane; j < units; j += 64) {
            const u32x4_t v = x[j];
            o[j] = v;
            s = fastnorm_fold<T>(v, s);
        }
        s = fastnorm_wave_sum(s);
        if (lane == 0) xn2[d] = s;
        wave_max = __builtin_fmaxf(wave_max, s);
        if constexpr (sizeof(T) == 4) {
            if (planes && d < planes_rows) {
                bf16_t* p = planes + (uint64_t)d * (2u * ldp);
                for (uint32_t j = lane; j < ldp; j += 64) {
                    const float f = j < ld ? src[j] : 0.0f;
                    const bf16_t hi = f32_to_bf16_rne(f);
                    const bf16_t lo = f32_to_bf16_rne(f - bf16_to_f32(hi));
                    bf16_t* q = p + (uint64_t)(j >> 6) * 128 + (j & 63);
                    q[0] = hi;
                    q[64] = lo;
                }
            }
        }
    }
    if (lane == 0 && wave_max > 0.0f) atomicMax(max_bits, __float_as_uint(wave_max));  // >= 0: uint order == float order
}

// ------------------------------------------------------------------ compact: gather the live rows of a chunk
// Rows [r0, r1) of the corpus (r0 % 32 == 0): live row s goes to out row word_base[s / 32] + (live rows below s in its
// word) - out_base, with its xnorm2 entry.  `out` is the staging buffer (out_base = the chunk's first destination) or
// the corpus itself (out_base = 0): the caller's plan (compact_plan.h) guarantees that the destination rows lie below
// r0 then, so no wave writes a row another one still has to read.  No __restrict__: source and destination may be one
// allocation.
__global__ __launch_bounds__(256) void compact_rows_kernel(const u32x4_t* rows, const float* xn2, const uint32_t* __restrict__ del,
                                                           const uint32_t* __restrict__ word_base, uint64_t r0, uint64_t r1,
                                                           uint32_t units, u32x4_t* out_rows, float* out_xn2, uint64_t out_base) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t r = r0 + wave; r < r1; r += nwaves) {
        const uint32_t w = del[r / 32], b = (uint32_t)(r % 32);
        if ((w >> b) & 1u) continue;
        const uint64_t d = (uint64_t)word_base[r / 32] + (uint32_t)__builtin_popcount(~w & ((1u << b) - 1u)) - out_base;
        const u32x4_t* x = rows + r * (uint64_t)units;
        u32x4_t* o = out_rows + d * (uint64_t)units;
        for (uint32_t j = lane; j < units; j += 64) o[j] = x[j];
        if (lane == 0) out_xn2[d] = xn2[r];
    }
}

// max of n squared norms (all >= 0, so the uint order of the bits is the float order) into *max_bits, which the caller cleared
__global__ __launch_bounds__(256) void xn2_max_kernel(const float* __restrict__ xn2, uint64_t n, uint32_t* __restrict__ max_bits) {
    float m = 0.0f;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        m = __builtin_fmaxf(m, xn2[i]);
    for (int o = 32; o > 0; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(max_bits, __float_as_uint(m));
}

// ------------------------------------------------------------------ launchers
// memory-bound: at most 2048 work-groups, the rest by the grid-stride loops
static inline unsigned rows_grid(uint64_t rows) { return (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(1, (rows + 3) / 4)); }

void launch_scatter_rows(const void* d_staged, const uint32_t* d_dst, uint64_t n, int dtype, uint32_t ld, void* d_corpus,
                         float* d_xn2, uint32_t* d_max_bits, void* d_planes, uint64_t planes_rows, uint32_t ldp, hipStream_t s) {
    if (!n) return;
    if (dtype == DT_BF16)
        scatter_rows_kernel<bf16_t><<<rows_grid(n), 256, 0, s>>>((const bf16_t*)d_staged, d_dst, n, ld, (bf16_t*)d_corpus, d_xn2,
                                                                 d_max_bits, nullptr, 0, 0);
    else
        scatter_rows_kernel<float><<<rows_grid(n), 256, 0, s>>>((const float*)d_staged, d_dst, n, ld, (float*)d_corpus, d_xn2,
                                                                d_max_bits, (bf16_t*)d_planes, planes_rows, ldp);
}

void launch_compact_rows(const void* d_rows, const float* d_xn2, const uint32_t* d_del, const uint32_t* d_word_base, uint64_t r0,
                         uint64_t r1, size_t row_bytes, void* d_out_rows, float* d_out_xn2, uint64_t out_base, hipStream_t s) {
    if (r1 <= r0) return;
    compact_rows_kernel<<<rows_grid(r1 - r0), 256, 0, s>>>((const u32x4_t*)d_rows, d_xn2, d_del, d_word_base, r0, r1,
                                                           (uint32_t)(row_bytes / 16), (u32x4_t*)d_out_rows, d_out_xn2, out_base);
}

void launch_xn2_max(const float* d_xn2, uint64_t n, uint32_t* d_max_bits, hipStream_t s) {
    if (!n) return;
    xn2_max_kernel<<<(unsigned)std::min<uint64_t>(1024, (n + 255) / 256), 256, 0, s>>>(d_xn2, n, d_max_bits);
}

}  // namespace vrod
