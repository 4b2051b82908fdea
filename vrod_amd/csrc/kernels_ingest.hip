// kernels_ingest.hip -- rows in device memory become prepared rows (gfx950): every add, update and upsert, host or
// _device form, and vrod_index_get_rows / _get_rows_device on the way out.
//
// The rows arrive typed (fp32, bf16 or fp16) and strided: a slice of an encoder's output tensor for the _device forms,
// the staged fp32 upload (or synthetic chunk) at stride dim for the host forms.  One kernel family turns them into
// prepared rows (kernels_prep.hip's spec, prep_chain.h's arithmetic), reading the source from HBM ONCE, coalesced.
// Host decisions (which loads a pointer allows, rows per work-group, LDS) are ingest_plan.h's.
//
//   COSINE     a wave (dim <= 4096: four rows per work-group) or the whole work-group (beyond) loads its row widened
//              to fp32 into LDS, one thread per row walks the canonical fp64 chain over it (prep_chain_lds, the chain
//              of prep_queries_kernel; a work-group's four chains in four lanes of one wave), and all of them write the
//              row divided and rounded, padding zeroed.
//   L2 / IP    no chain, no LDS: a streaming convert-check-write, a wave per row.
//
// LDS and occupancy: 4 rows x dim x 4 B is 12 KiB at dim 768, so the 2048 threads of a CU (8 work-groups) fit its 160 KiB
// and the chains of 8 waves per CU hide behind each other and behind the loads of the next rows.
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "prep_chain.h"
#include "ingest_plan.h"

namespace vrod {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ widening, exact
template <int SRC> struct SrcElem { typedef uint16_t type; };
template <> struct SrcElem<SRC_F32> { typedef float type; };

// fp16 bits -> fp32, on the bits: exact for every encoding (subnormals m * 2^-24, -0.0, Inf and NaN kept as such) and
// independent of the wave's denormal mode
__device__ inline float f16_bits_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 0) {
        const float f = (float)m * 5.9604644775390625e-8f;   // m * 2^-24: both factors and the product are exact
        return __uint_as_float(__float_as_uint(f) | sign);
    }
    if (e == 31) return __uint_as_float(sign | 0x7F800000u | (m << 13));
    return __uint_as_float(sign | ((e + 112u) << 23) | (m << 13));
}
template <int SRC>
__device__ inline float widen16(uint16_t h) {
    if constexpr (SRC == SRC_BF16) return bf16_to_f32(h);
    else return f16_bits_to_f32(h);
}
template <int SRC>
__device__ inline float widen(typename SrcElem<SRC>::type x) {
    if constexpr (SRC == SRC_F32) return x;
    else return widen16<SRC>(x);
}
// the 16 / sizeof(element) values of one 16-B load
template <int SRC>
__device__ inline void widen_vec(u32x4_t w, float* f) {
    if constexpr (SRC == SRC_F32) {
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(w[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[2 * e] = widen16<SRC>((uint16_t)(w[e] & 0xFFFFu));
            f[2 * e + 1] = widen16<SRC>((uint16_t)(w[e] >> 16));
        }
    }
}

struct IngestArgs {
    const void* src;        // n (or more, under pick) rows of dim elements, row i at element i * stride
    uint64_t stride;
    const uint64_t* pick;   // null: row r of the launch is source row r; else source row pick[r]
    uint64_t n;
    uint32_t dim, ld, pitch;   // pitch: floats between the LDS rows of a work-group
    float* out_f32;         // exactly one of the two: [n][ld] prepared rows
    bf16_t* out_bf16;
    uint32_t* bad_flag;
};

__device__ inline void emit(const IngestArgs& a, uint64_t r, uint32_t j, float v) {
    if (a.out_bf16) a.out_bf16[r * a.ld + j] = f32_to_bf16_rne(v);
    else a.out_f32[r * a.ld + j] = v;
}
// V consecutive values from element j0 (j0 % V == 0: the stores are as aligned as the loads were)
template <int V>
__device__ inline void emit_vec(const IngestArgs& a, uint64_t r, uint32_t j0, const float* f) {
    if (a.out_bf16) {
        uint32_t w[V / 2];
#pragma unroll
        for (int e = 0; e < V / 2; ++e) w[e] = (uint32_t)f32_to_bf16_rne(f[2 * e]) | ((uint32_t)f32_to_bf16_rne(f[2 * e + 1]) << 16);
        bf16_t* o = a.out_bf16 + r * a.ld + j0;
        if constexpr (V == 4) { u32x2_t p; p[0] = w[0]; p[1] = w[1]; *reinterpret_cast<u32x2_t*>(o) = p; }
        else { u32x4_t p; p[0] = w[0]; p[1] = w[1]; p[2] = w[2]; p[3] = w[3]; *reinterpret_cast<u32x4_t*>(o) = p; }
    } else {
        float* o = a.out_f32 + r * a.ld + j0;
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            f32x4_t p;
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = f[4 * q + e];
            *reinterpret_cast<f32x4_t*>(o + 4 * q) = p;
        }
    }
}

// ------------------------------------------------------------------ typed, strided rows -> prepared rows
// GS threads share a row: a wave (four rows per work-group) or the work-group.  WIDE: every row starts on a 16-B boundary.
template <int SRC, bool NORMALISE, bool WIDE, int GS>
__global__ __launch_bounds__(256) void ingest_rows_kernel(IngestArgs a) {
    typedef typename SrcElem<SRC>::type E;
    constexpr int V = 16 / (int)sizeof(E);
    constexpr uint32_t RPG = 256 / GS;
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [RPG][pitch], NORMALISE only
    __shared__ double s_nrm[4];
    const uint32_t g = threadIdx.x / GS, t = threadIdx.x % GS;
    const uint32_t nvec = WIDE ? a.dim / V : 0u;   // whole 16-B units of a row; the rest goes element by element
    bool bad = false;
    // (the trip count depends on the block alone: every thread reaches every barrier)
    for (uint64_t base = (uint64_t)blockIdx.x * RPG; base < a.n; base += (uint64_t)gridDim.x * RPG) {
        const uint64_t r = base + g;
        const bool live = r < a.n;
        const E* x = static_cast<const E*>(a.src) + (live ? (a.pick ? a.pick[r] : r) * a.stride : 0);
        if constexpr (NORMALISE) {
            float* row = lds + g * a.pitch;
            if (live) {
                for (uint32_t jv = t; jv < nvec; jv += GS) {
                    float f[V];
                    widen_vec<SRC>(reinterpret_cast<const u32x4_t*>(x)[jv], f);
#pragma unroll
                    for (int q = 0; q < V / 4; ++q) {
                        f32x4_t p;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { p[e] = f[4 * q + e]; bad |= prep_is_bad(p[e]); }
                        *reinterpret_cast<f32x4_t*>(row + jv * V + 4 * q) = p;
                    }
                }
                for (uint32_t j = nvec * V + t; j < a.dim; j += GS) {
                    const float f = widen<SRC>(x[j]);
                    bad |= prep_is_bad(f);
                    row[j] = f;
                }
            }
            __syncthreads();
            // The chains of the group's rows walk side by side in the first lanes of ONE wave: a chain step takes a wave
            // its fp64 issue slots whatever the number of lanes in it, and those slots are what bounds this kernel.
            if (threadIdx.x < RPG && base + threadIdx.x < a.n)
                s_nrm[threadIdx.x] = __builtin_sqrt(prep_chain_lds(lds + threadIdx.x * a.pitch, a.dim));
            __syncthreads();
            if (live) {
                const double nrm = s_nrm[g];
                for (uint32_t j = t; j < a.ld; j += GS) emit(a, r, j, j < a.dim ? prep_scale(row[j], nrm) : 0.0f);
            }
            __syncthreads();   // the next row's loads overwrite this one
        } else {
            if (!live) continue;
            for (uint32_t jv = t; jv < nvec; jv += GS) {
                float f[V];
                widen_vec<SRC>(reinterpret_cast<const u32x4_t*>(x)[jv], f);
#pragma unroll
                for (int e = 0; e < V; ++e) bad |= prep_is_bad(f[e]);
                emit_vec<V>(a, r, jv * V, f);
            }
            for (uint32_t j = nvec * V + t; j < a.ld; j += GS) {
                float f = 0.0f;
                if (j < a.dim) { f = widen<SRC>(x[j]); bad |= prep_is_bad(f); }
                emit(a, r, j, f);
            }
        }
    }
    if (bad) atomicOr(a.bad_flag, 1u);
}

// ------------------------------------------------------------------ strided rows -> dense rows of the same type
// The first leg of a source that lives on another device than the shard: packed here, on the source's device, copied
// peer to peer, and ingested from the dense copy.
template <typename E>
__global__ __launch_bounds__(256) void ingest_pack_kernel(const E* __restrict__ src, uint64_t stride, const uint64_t* __restrict__ pick,
                                                          uint64_t n, uint32_t dim, E* __restrict__ out) {
    const uint64_t total = n * (uint64_t)dim;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / dim;
        const uint32_t j = (uint32_t)(i - r * dim);
        out[i] = src[(pick ? pick[r] : r) * stride + j];
    }
}

// ------------------------------------------------------------------ stored rows -> fp32 rows at a pitch
// Stored rows widened back to fp32, out_stride (>= dim) floats apart; the padding between the rows is not written.
template <typename T>
__global__ __launch_bounds__(256) void rows_get_strided_kernel(const T* __restrict__ rows, uint64_t n, uint32_t dim, uint32_t ld,
                                                               float* __restrict__ out, uint64_t out_stride) {
    const uint64_t total = n * (uint64_t)dim;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / dim;
        const uint32_t j = (uint32_t)(i - r * dim);
        if constexpr (sizeof(T) == 2) out[r * out_stride + j] = bf16_to_f32(rows[r * (uint64_t)ld + j]);
        else out[r * out_stride + j] = rows[r * (uint64_t)ld + j];
    }
}

// ------------------------------------------------------------------ launchers
static inline unsigned ingest_grid(uint64_t groups) {
    const uint64_t cap = 256ull * 8;   // 8 work-groups of 256 threads fill a CU
    return (unsigned)(groups < 1 ? 1 : groups > cap ? cap : groups);
}

template <int SRC, bool NORMALISE, bool WIDE, int GS>
static void launch_ingest_as(const IngestArgs& a, hipStream_t s) {
    const size_t lds = NORMALISE ? (size_t)(256 / GS) * a.pitch * sizeof(float) : 0;
    // One row of VROD_MAX_DIM floats is 128 KiB, beside the kernel's static words.  A function attribute belongs to the
    // current device, so it is set with every launch that needs it, not once per process.
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)ingest_rows_kernel<SRC, NORMALISE, WIDE, GS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            128 * 1024) != hipSuccess)
        (void)hipGetLastError();   // (the launch reports what it cannot have)
    const uint64_t rpg = 256 / GS;
    ingest_rows_kernel<SRC, NORMALISE, WIDE, GS><<<ingest_grid((a.n + rpg - 1) / rpg), 256, lds, s>>>(a);
}
template <int SRC>
static void launch_ingest_src(const IngestArgs& a, bool normalise, bool wide, bool per_wave, hipStream_t s) {
    if (!normalise) {
        if (wide) launch_ingest_as<SRC, false, true, 64>(a, s);
        else launch_ingest_as<SRC, false, false, 64>(a, s);
    } else if (per_wave) {
        if (wide) launch_ingest_as<SRC, true, true, 64>(a, s);
        else launch_ingest_as<SRC, true, false, 64>(a, s);
    } else {
        if (wide) launch_ingest_as<SRC, true, true, 256>(a, s);
        else launch_ingest_as<SRC, true, false, 256>(a, s);
    }
}

void launch_ingest_rows(const void* d_src, int src_dtype, uint64_t row_stride, const uint64_t* d_pick, uint64_t n, uint32_t dim,
                        uint32_t ld, int metric, int dtype, uint32_t* d_bad_flag, void* d_out, hipStream_t s) {
    if (!n) return;
    IngestArgs a{};
    a.src = d_src;
    a.stride = row_stride;
    a.pick = d_pick;
    a.n = n;
    a.dim = dim;
    a.ld = ld;
    a.pitch = ingest_lds_pitch(dim);
    a.out_f32 = dtype == DT_BF16 ? nullptr : (float*)d_out;
    a.out_bf16 = dtype == DT_BF16 ? (bf16_t*)d_out : nullptr;
    a.bad_flag = d_bad_flag;
    const bool wide = ingest_load_bytes((uint64_t)(uintptr_t)d_src, src_dtype, row_stride) == 16;
    const bool per_wave = ingest_rows_per_group(dim) == 4;
    const bool normalise = metric == M_COSINE;
    if (src_dtype == SRC_F32) launch_ingest_src<SRC_F32>(a, normalise, wide, per_wave, s);
    else if (src_dtype == SRC_BF16) launch_ingest_src<SRC_BF16>(a, normalise, wide, per_wave, s);
    else launch_ingest_src<SRC_F16>(a, normalise, wide, per_wave, s);
}

void launch_ingest_pack(const void* d_src, int src_dtype, uint64_t row_stride, const uint64_t* d_pick, uint64_t n, uint32_t dim,
                        void* d_out, hipStream_t s) {
    if (!n) return;
    const unsigned g = ingest_grid((n * (uint64_t)dim + 255) / 256);
    if (src_dtype == SRC_F32) ingest_pack_kernel<float><<<g, 256, 0, s>>>((const float*)d_src, row_stride, d_pick, n, dim, (float*)d_out);
    else ingest_pack_kernel<uint16_t><<<g, 256, 0, s>>>((const uint16_t*)d_src, row_stride, d_pick, n, dim, (uint16_t*)d_out);
}

void launch_rows_get_strided(const void* d_rows, int dtype, uint64_t n, uint32_t dim, uint32_t ld, float* d_out, uint64_t out_stride,
                             hipStream_t s) {
    if (!n) return;
    const unsigned g = ingest_grid((n * (uint64_t)dim + 255) / 256);
    if (dtype == DT_BF16) rows_get_strided_kernel<bf16_t><<<g, 256, 0, s>>>((const bf16_t*)d_rows, n, dim, ld, d_out, out_stride);
    else rows_get_strided_kernel<float><<<g, 256, 0, s>>>((const float*)d_rows, n, dim, ld, d_out, out_stride);
}

}  // namespace vrod
