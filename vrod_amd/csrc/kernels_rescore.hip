// kernels_rescore.hip -- canonical (oracle-order) re-score on gfx950.
//
// The fast passes (kernels_stream.hip, kernels_mfma.hip) accumulate in whatever order is
// fastest.  vRod's data model is a plain Vec<Vec<f32>> walked by one thread
// (reference src/utils/embeddings.rs:29, src/command/types.rs:10), so the result contract
// (DESIGN.md "Scan spec", oracle/vrod_oracle.c orc_dot_canonical / orc_l2_canonical) is the
// strictly sequential fp32 chain   acc = acc + (q[j] * x[j])   with the product and the
// sum each rounded to fp32 -- no FMA, no reassociation.  This kernel recomputes exactly
// that chain for the few candidates the fast pass selected, so ids AND score bits equal
// the oracle's.  v_mul_f32 / v_add_f32 / v_sub_f32 are issued through inline asm so that
// no compiler contraction (hipcc defaults to -ffp-contract=fast) can fuse them.
//
// Layout: one lane owns one (query, candidate row) chain.  A wave stages 64 candidate
// rows x 64 elements through an LDS tile (coalesced 256-B / 128-B row segments in,
// 16-B column walk out: row stride 68 dwords).
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "rescore_chain.h"

namespace vrod {

// One wave per block: the block owns candidate slots [64*blockIdx.x, +64) of query blockIdx.y
// (rows from d_cand_rows, ~0u = empty; empties sit at the end of a list).
// Each 64-element chunk of the 64 rows is fetched with 16-B loads, all issued before the
// first LDS write (the chain itself is sequential, the loads must not be), and then every
// lane walks its own row of the tile in order.
template <typename T, int METRIC>
__global__ __launch_bounds__(64) void rescore_kernel(const T* __restrict__ corpus, uint32_t dim,
                                                     uint32_t ld, const float* __restrict__ q,
                                                     const uint32_t* __restrict__ cand_rows,
                                                     uint32_t kp, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* q_lds = smem;                       // [ld]
    float* tile = smem + ld;                   // [64][68]
    const int lane = threadIdx.x;

    const uint32_t qi = blockIdx.y;
    const float* qrow = q + (uint64_t)qi * ld;
    for (uint32_t i = lane; i < ld; i += 64) q_lds[i] = qrow[i];

    const uint64_t slot = (uint64_t)blockIdx.x * 64 + lane;
    uint32_t my_row = slot < kp ? cand_rows[(uint64_t)qi * kp + slot] : 0xFFFFFFFFu;
    const bool valid = my_row != 0xFFFFFFFFu;
    if (!valid) my_row = 0u;
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0ull) return;  // whole wave idle (single-wave block: no barrier is skipped)
    // valid slots are a prefix of the wave; rows beyond it are not fetched
    const float acc = canonical_chain_wave<T, METRIC>(corpus, dim, ld, q_lds, tile, my_row, 64 - __builtin_clzll(vmask));
    if (slot < kp) out[(uint64_t)qi * kp + slot] = valid ? acc : __uint_as_float(kScoreNoneBits);
}

// ---------------------------------------------------------------------------------------
// Exact path: the canonical score of EVERY row for NQ queries at once (the queries whose
// certificate failed).  One pass over the shard serves NQ chains per lane: the corpus chunk is
// staged once, and the NQ dependent add chains are independent of each other, so they fill the
// latency a single chain leaves idle (one query: ~64 serial adds per chunk per lane).
// A query element is the same for all 64 rows of the wave: lane l of a VGPR holds q[j0 + l], and
// v_readlane moves it to an SGPR operand of the product -- NQ query rows in LDS would cost a
// 16-B broadcast read per 4 elements per query (LDS-bound at 8 queries) and 3 waves per CU.
// out[n * out_ld + row], n = position of the query in `qs`.
struct RescoreQuerySet { uint32_t qi[8]; };
template <int I> struct RingSlot { static constexpr int value = I; };

__device__ __forceinline__ float mul_rn_s(float s, float b) {
    float r;
    asm("v_mul_f32_e32 %0, %1, %2" : "=v"(r) : "s"(s), "v"(b));
    return r;
}
__device__ __forceinline__ float sub_rn_s(float s, float b) {
    float r;
    asm("v_sub_f32_e32 %0, %1, %2" : "=v"(r) : "s"(s), "v"(b));
    return r;
}

//
// One body serves three kernels.  The block's 64 rows are rows [row0, row0 + 64) of `nrows` -- of the corpus, or
// (LIST) of the ascending row list `list` -- and its NQ chains are the queries qs.qi[0..NQ) of `q`; chain n < n_write
// goes to out[n * out_ld + row0 + lane].  `tile` is the block's [64][kTileStride] LDS staging tile.
template <typename T, int METRIC, int NQ, bool LIST>
__device__ __forceinline__ void rescore_all_body(const T* __restrict__ corpus, uint32_t dim, uint32_t ld, const float* __restrict__ q,
                                                 const RescoreQuerySet& qs, uint64_t nrows, uint64_t row0, float* __restrict__ out,
                                                 uint64_t out_ld, const uint32_t* __restrict__ list, int n_write, float* tile) {
    constexpr int EPU = 16 / (int)sizeof(T);
    constexpr int LPC = 64 / EPU;
    constexpr int RPI = 64 / LPC;
    constexpr int NI = 64 / RPI;
    const int lane = threadIdx.x;
    const uint64_t slot = row0 + lane;
    const bool valid = slot < nrows;
    const int nvalid = nrows - row0 < 64 ? (int)(nrows - row0) : 64;   // rows are a prefix of the wave
    const int ni_used = (nvalid + RPI - 1) / RPI;
    const int sub = lane / LPC, part = lane % LPC;

    float acc[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) acc[n] = 0.0f;
    // ring depth: a bf16 chunk of 64 rows is 8 KB (8 x 16 B per lane), an fp32 chunk 16 KB
    constexpr int D = sizeof(T) == 4 ? 2 : 3;
    u32x4 v[D][NI];
    float vq[D][NQ];
    auto fetch = [&](u32x4 (&vs)[NI], float (&qv)[NQ], uint32_t j0) {
        const uint32_t e0 = j0 + part * EPU;
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            vs[it] = u32x4{0u, 0u, 0u, 0u};
            if (it < ni_used) {
                uint64_t row = row0 + it * RPI + sub;
                if (row >= nrows) row = row0;
                if constexpr (LIST) row = list[row];
                if (e0 < ld) vs[it] = *reinterpret_cast<const u32x4*>(corpus + row * ld + e0);
            }
        }
#pragma unroll
        for (int n = 0; n < NQ; ++n) qv[n] = j0 + lane < ld ? q[(uint64_t)qs.qi[n] * ld + j0 + lane] : 0.0f;
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if ((uint32_t)d * 64 < dim) fetch(v[d], vq[d], d * 64);
    // one ring slot per call, the slot a compile-time constant (a `#pragma unroll` over d is
    // refused for the largest variants, and a runtime d would put the ring into scratch)
    auto chunk = [&](auto dc, uint32_t jb) __attribute__((always_inline)) -> bool {
            constexpr int d = decltype(dc)::value;
            const uint32_t j0 = jb + d * 64;
            if (j0 >= dim) return false;
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
            float qc[NQ];
#pragma unroll
            for (int n = 0; n < NQ; ++n) qc[n] = vq[d][n];
            if (j0 + 64 * D < dim) fetch(v[d], vq[d], j0 + 64 * D);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t jn = dim - j0 < 64 ? dim - j0 : 64;
            const float* trow = tile + lane * kTileStride;
            // elements [0, jn) of the chunk; the tail chunk's padding (x = q = 0 beyond dim) is
            // NOT walked: acc + (+0 * +0) would turn an accumulated -0.0 into +0.0
#pragma unroll
            for (uint32_t l = 0; l < 64; l += 4) {
                if (l < jn) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(trow + l);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (l + e < jn) {
#pragma unroll
                            for (int n = 0; n < NQ; ++n) {
                                const float qs_ = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qc[n]), (int)(l + e)));
                                if constexpr (METRIC == M_COSINE) {
                                    acc[n] = add_rn(acc[n], mul_rn_s(qs_, x[e]));
                                } else {
                                    const float dd = sub_rn_s(qs_, x[e]);
                                    acc[n] = add_rn(acc[n], mul_rn(dd, dd));
                                }
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            return true;
    };
    for (uint32_t jb = 0; jb < dim; jb += 64 * D) {
        if (!chunk(RingSlot<0>{}, jb)) break;
        if (!chunk(RingSlot<1>{}, jb)) break;
        if constexpr (D == 3)
            if (!chunk(RingSlot<2>{}, jb)) break;
    }
    if (valid) {
#pragma unroll
        for (int n = 0; n < NQ; ++n)
            if (n < n_write) out[(uint64_t)n * out_ld + slot] = acc[n];
    }
}

// Exact path (LIST false): block b takes corpus rows [64 b, 64 b + 64) and the NQ queries of `qs`.
// LIST (the gather path of a filtered search, rescore_list): the same chains over the rows a list names -- column c is
// row list[c], c < nrows -- for a whole block of `nq_list` consecutive queries of `q`.  Block b takes query group
// b % n_qgroups (NQ queries; a short last group repeats its last query and writes only its own) and list tile
// b / n_qgroups, so that the blocks in flight together share their 64 rows through L2.
template <typename T, int METRIC, int NQ, bool LIST>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void rescore_all_kernel(const T* __restrict__ corpus, uint32_t dim, uint32_t ld,
                                                         const float* __restrict__ q, RescoreQuerySet qs,
                                                         uint64_t nrows, float* __restrict__ out, uint64_t out_ld,
                                                         const uint32_t* __restrict__ list, uint32_t nq_list, uint32_t n_qgroups) {
    __shared__ __attribute__((aligned(16))) float tile[64 * kTileStride];
    const uint32_t qg = LIST ? blockIdx.x % n_qgroups : 0u;
    const uint64_t row0 = (uint64_t)(LIST ? blockIdx.x / n_qgroups : blockIdx.x) * 64;
    int n_write = NQ;
    if constexpr (LIST) {
#pragma unroll
        for (int n = 0; n < NQ; ++n) qs.qi[n] = qg * NQ + n < nq_list ? qg * NQ + n : nq_list - 1;
        n_write = (int)(nq_list - qg * NQ < (uint32_t)NQ ? nq_list - qg * NQ : (uint32_t)NQ);
        out += (uint64_t)qg * NQ * out_ld;
    }
    rescore_all_body<T, METRIC, NQ, LIST>(corpus, dim, ld, q, qs, nrows, row0, out, out_ld, list, n_write, tile);
}

// SEGMENTED (a labelled search, label_plan.h): one launch scores many (label, queries) groups, each over its own
// segment of one row-list buffer.  Block b finds its entry of the work table (seg_lookup: a binary search over the
// entries' first blocks, uniform across the wave), then takes one subgroup of the entry's queries -- `nqc` of them per
// lane, the entry's class -- and one 64-row tile of its segment; consecutive blocks are the subgroups of one tile, so the
// blocks in flight together share its rows through L2.  Query n of a subgroup is prepared row slot_q[slot] of `q`; a
// short last subgroup repeats its last query and writes only its own.  out[(slot - slot_first) * out_ld + column].
template <typename T, int METRIC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void rescore_segments_kernel(
    const T* __restrict__ corpus, uint32_t dim, uint32_t ld, const float* __restrict__ q, const SegEntry* __restrict__ entries,
    uint32_t n_entries, const uint32_t* __restrict__ slot_q, uint32_t slot_first, const uint32_t* __restrict__ lists,
    float* __restrict__ out, uint64_t out_ld) {
    __shared__ __attribute__((aligned(16))) float tile[64 * kTileStride];
    const SegBlock w = seg_lookup(entries, n_entries, blockIdx.x);
    const SegEntry e = entries[w.entry];
    const uint32_t s0 = e.slot0 + w.sub * e.nqc;               // first slot of the subgroup
    const uint32_t left = e.nq - w.sub * e.nqc;                 // its queries (>= 1), capped by the class below
    RescoreQuerySet qs;
#pragma unroll
    for (uint32_t n = 0; n < 8; ++n) qs.qi[n] = slot_q[s0 + (n < left ? n : left - 1)];
    const uint32_t* list = lists + e.list_base;
    float* o = out + (uint64_t)(s0 - slot_first) * out_ld;
    const uint64_t row0 = (uint64_t)w.tile * 64;
    const int n_write = (int)(left < e.nqc ? left : e.nqc);
    switch (e.nqc) {
        case 1: rescore_all_body<T, METRIC, 1, true>(corpus, dim, ld, q, qs, e.m, row0, o, out_ld, list, n_write, tile); break;
        case 2: rescore_all_body<T, METRIC, 2, true>(corpus, dim, ld, q, qs, e.m, row0, o, out_ld, list, n_write, tile); break;
        case 4: rescore_all_body<T, METRIC, 4, true>(corpus, dim, ld, q, qs, e.m, row0, o, out_ld, list, n_write, tile); break;
        default: rescore_all_body<T, METRIC, 8, true>(corpus, dim, ld, q, qs, e.m, row0, o, out_ld, list, n_write, tile); break;
    }
}

static void launch_rescore(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld,
                           const float* d_q, int nq, const uint32_t* d_cand_rows, uint32_t kp,
                           float* d_out, hipStream_t s) {
    const size_t lds = ((size_t)ld + 64 * kTileStride) * sizeof(float);
    dim3 grid((kp + 63) / 64, nq);
#define VROD_RS(TT, MM) rescore_kernel<TT, MM><<<grid, 64, lds, s>>>((const TT*)d_corpus, dim, ld, d_q, d_cand_rows, kp, d_out)
    if (dtype == DT_BF16) { if (metric == M_COSINE) VROD_RS(bf16_t, M_COSINE); else VROD_RS(bf16_t, M_L2); }
    else { if (metric == M_COSINE) VROD_RS(float, M_COSINE); else VROD_RS(float, M_L2); }
#undef VROD_RS
}

void launch_rescore_candidates(const void* d_corpus, int dtype, int metric, uint32_t dim,
                               uint32_t ld, const float* d_q, int nq, const uint32_t* d_cand_rows,
                               uint32_t kp, float* d_out, hipStream_t s) {
    if (!nq || !kp) return;
    launch_rescore(d_corpus, dtype, metric, dim, ld, d_q, nq, d_cand_rows, kp, d_out, s);
}

int rescore_all_max_queries(uint32_t) { return 8; }

void launch_rescore_all(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld,
                        const float* d_q, const uint32_t* query_index, int nq, uint64_t nrows,
                        float* d_out, uint64_t out_ld, hipStream_t s) {
    if (!nrows || nq <= 0) return;
    RescoreQuerySet qs;
    for (int i = 0; i < 8; ++i) qs.qi[i] = query_index[i < nq ? i : nq - 1];
    const unsigned grid = (unsigned)((nrows + 63) / 64);
#define VROD_RA(TT, MM, NN) rescore_all_kernel<TT, MM, NN, false><<<grid, 64, 0, s>>>((const TT*)d_corpus, dim, ld, d_q, qs, nrows, d_out, out_ld, nullptr, 0u, 1u)
#define VROD_RA_N(TT, MM)                                                                           \
    switch (nq) {                                                                                   \
        case 1: VROD_RA(TT, MM, 1); break;                                                          \
        case 2: VROD_RA(TT, MM, 2); break;                                                          \
        case 4: VROD_RA(TT, MM, 4); break;                                                          \
        default: VROD_RA(TT, MM, 8); break;                                                         \
    }
    if (dtype == DT_BF16) { if (metric == M_COSINE) { VROD_RA_N(bf16_t, M_COSINE) } else { VROD_RA_N(bf16_t, M_L2) } }
    else { if (metric == M_COSINE) { VROD_RA_N(float, M_COSINE) } else { VROD_RA_N(float, M_L2) } }
#undef VROD_RA_N
#undef VROD_RA
}

void launch_rescore_list(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q, uint32_t nq,
                         const uint32_t* d_list, uint64_t m, float* d_out, uint64_t out_ld, hipStream_t s) {
    if (!m || !nq) return;
    RescoreQuerySet qs{};
    const int nqb = nq >= 8 ? 8 : nq >= 4 ? 4 : nq >= 2 ? 2 : 1;   // queries per lane: 8 once the batch has them
    const uint32_t n_qgroups = (nq + nqb - 1) / nqb;
    const unsigned grid = (unsigned)(((m + 63) / 64) * n_qgroups);
#define VROD_RL(TT, MM, NN) rescore_all_kernel<TT, MM, NN, true><<<grid, 64, 0, s>>>((const TT*)d_corpus, dim, ld, d_q, qs, m, d_out, out_ld, d_list, nq, n_qgroups)
#define VROD_RL_N(TT, MM)                                                                           \
    switch (nqb) {                                                                                  \
        case 1: VROD_RL(TT, MM, 1); break;                                                          \
        case 2: VROD_RL(TT, MM, 2); break;                                                          \
        case 4: VROD_RL(TT, MM, 4); break;                                                          \
        default: VROD_RL(TT, MM, 8); break;                                                         \
    }
    if (dtype == DT_BF16) { if (metric == M_COSINE) { VROD_RL_N(bf16_t, M_COSINE) } else { VROD_RL_N(bf16_t, M_L2) } }
    else { if (metric == M_COSINE) { VROD_RL_N(float, M_COSINE) } else { VROD_RL_N(float, M_L2) } }
#undef VROD_RL_N
#undef VROD_RL
}

void launch_rescore_segments(const void* d_corpus, int dtype, int metric, uint32_t dim, uint32_t ld, const float* d_q,
                             const SegEntry* d_entries, uint32_t n_entries, uint32_t n_blocks, const uint32_t* d_slot_q, uint32_t slot_first,
                             const uint32_t* d_lists, float* d_out, uint64_t out_ld, hipStream_t s) {
    if (!n_entries || !n_blocks) return;
#define VROD_RG(TT, MM) rescore_segments_kernel<TT, MM><<<n_blocks, 64, 0, s>>>((const TT*)d_corpus, dim, ld, d_q, d_entries, n_entries, d_slot_q, slot_first, d_lists, d_out, out_ld)
    if (dtype == DT_BF16) { if (metric == M_COSINE) VROD_RG(bf16_t, M_COSINE); else VROD_RG(bf16_t, M_L2); }
    else { if (metric == M_COSINE) VROD_RG(float, M_COSINE); else VROD_RG(float, M_L2); }
#undef VROD_RG
}

}  // namespace vrod
