// centroid_plan.h -- the arithmetic of group centroids (vrod_index_centroids_where): the scale of the exact integer sum,
// the quantiser of an element, the two conversions of a sum back to fp32, the workspace layout and the launch geometry.
// Plain arithmetic, no HIP headers (aggregate_plan.h): vrod_index.hip enqueues what these functions decide,
// kernels_centroid.hip calls the VROD_TAG_HD ones on the device, tests/test_centroid_plan.py compiles this header as
// host C++.
//
// The value (DESIGN.md "Group centroids").  x: an element as vrod_index_get_rows reads it.  n: the handle's rows, deleted
// ones included; R: the smallest integer with n < 2^R.  E: 1 on a COSINE handle (|x| < 2), else from m, the largest
// bits(x) & 0x7fffffff among the considered rows, E = max(m >> 23, 1) - 126, so that every |x| < 2^E.  s = 62 - R - E.
//   q = llrint((double)x * 2^s)        the product is exact in fp64, ties go to even, |q| <= 2^(62 - R)
//   S = the sum of q over the group    in int64: fewer than 2^R rows, so |S| < 2^62 -- exact, commutative, no wrap
//   sum  = (float)((double)S * 2^-s)
//   mean = (float)(((double)S / (double)count) * 2^-s)
// Nothing here depends on the order the rows are added in, so the kernels may fold partial sums anywhere.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "aggregate_plan.h"   // the group table the ranks are found in (and VROD_TAG_HD, the row-predicate geometry)

namespace vrod {

constexpr uint32_t kCentroidSum = 8;                 // VROD_CENTROID_SUM
constexpr uint32_t kCentroidMaxGroups = 1u << 16;    // VROD_MAX_CENTROID_GROUPS
// The layout of vrod_centroid_group (include/vrod.h): 24 bytes, no padding.
struct CentroidGroup { int64_t key; uint64_t count, first_id; };

constexpr uint32_t kCentroidNonFinite = 0x7f800000u;   // m at or above this: an infinity or a NaN among the considered rows
constexpr uint32_t kCentroidNoRank = UINT32_MAX;       // a table slot that holds no group of the call

// R: the smallest integer with n < 2^R (0 for an empty handle, 12 for 4095 rows, 13 for 4096).
inline int32_t centroid_row_bits(uint64_t n) {
    int32_t r = 0;
    while (r < 64 && (n >> r) != 0) ++r;
    return r;
}
// E from m = max(bits(x) & 0x7fffffff), m < kCentroidNonFinite: every |x| < 2^E.  Subnormals and zeros share the
// exponent field 0 with the scale of field 1.
inline int32_t centroid_exponent(uint32_t m) {
    const int32_t e = (int32_t)(m >> 23);
    return (e > 1 ? e : 1) - 126;
}
// A prepared COSINE row is finite with |x| <= 1, whatever was added: the ingest refuses NaN and infinities, the norm of
// finite fp32 values is taken in fp64 and cannot overflow, and a zero row stays zero (prep_chain.h).  So no stored cosine
// element is non-finite, and the COSINE scale needs no pass over the rows.
constexpr int32_t kCentroidCosineExponent = 1;
inline int32_t centroid_scale(int32_t R, int32_t E) { return 62 - R - E; }

// q = llrint((double)x * 2^s) of the fp32 with these bits, in integer arithmetic: x = +-m24 * 2^(max(e, 1) - 150), so q
// is m24 shifted by sh = max(e, 1) - 150 + s -- to the left exactly, to the right with the dropped bits rounded to
// nearest, ties to even.  With |x| < 2^E and s = 62 - R - E the left shift is at most 38 - R.  Finite x only.
VROD_TAG_HD inline int64_t centroid_quantise(uint32_t bits, int32_t s) {
    const uint32_t e = (bits >> 23) & 0xffu;
    const uint32_t m24 = (bits & 0x7fffffu) | (e ? 0x800000u : 0u);
    const int32_t sh = (int32_t)(e ? e : 1u) - 150 + s;
    int64_t q;
    if (sh >= 0) {
        q = (int64_t)((uint64_t)m24 << (sh & 63));
    } else if (sh < -25) {
        q = 0;   // below a quarter of a quantum
    } else {
        const uint32_t n = (uint32_t)-sh;   // 1 .. 25, m24 < 2^24
        const uint32_t fl = m24 >> n, rem = m24 & ((1u << n) - 1u), half = 1u << (n - 1u);
        q = (int64_t)(fl + ((rem > half || (rem == half && (fl & 1u))) ? 1u : 0u));
    }
    return (bits >> 31) ? -q : q;
}

// 2^k as a double, -1022 <= k <= 1023 (s lies within -106 .. 186).
VROD_TAG_HD inline double centroid_pow2(int32_t k) {
    const uint64_t b = (uint64_t)(k + 1023) << 52;
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
// The two outputs: each conversion and the division one IEEE round-to-nearest-even operation, the products by a power
// of two exact.  S == 0 gives +0.0f.
VROD_TAG_HD inline float centroid_sum_value(int64_t S, int32_t s) { return (float)((double)S * centroid_pow2(-s)); }
VROD_TAG_HD inline float centroid_mean_value(int64_t S, uint64_t count, int32_t s) {
    return (float)(((double)S / (double)count) * centroid_pow2(-s));
}

// The small workspace of one call, beside the accumulators ([groups][dim] int64): the max word, the ordered groups'
// keys and counts, and the rank of every slot of the aggregation's table (aggregate_plan.h: slots + 1 of them).
struct CentroidWs {
    uint32_t* max_bits;   // [2]: m, and a word of padding
    int64_t* keys;        // [groups] ascending
    uint64_t* counts;     // [groups]
    uint32_t* rank;       // [slots + 1]: the rank of the slot's key among the groups, or kCentroidNoRank
};
inline size_t centroid_ws_bytes(uint64_t groups, uint64_t slots) { return 8 + (size_t)groups * 16 + (size_t)(slots + 1) * 4; }
inline CentroidWs centroid_ws_view(void* base, uint64_t groups) {
    CentroidWs w;
    w.max_bits = (uint32_t*)base;
    w.keys = (int64_t*)((char*)base + 8);
    w.counts = (uint64_t*)(w.keys + groups);
    w.rank = (uint32_t*)(w.counts + groups);
    return w;
}
inline size_t centroid_acc_bytes(uint64_t groups, uint32_t dim) { return (size_t)groups * dim * 8; }

// Launch geometry: the row-predicate passes' -- a work-group owns kRowPredRowsPerGroup rows and reads their 64 hit words.
// A row is read in 16-byte pieces (8 bf16 or 4 fp32 elements), a lane a piece; a team of lanes -- the power of two at or
// above the pieces of a row, at most the work-group -- walks a contiguous part of the work-group's hit list.
constexpr uint32_t kCentroidThreads = kRowPredThreads;
constexpr uint32_t kCentroidInFlight = 4;   // rows a lane loads before it adds them
inline uint32_t centroid_elems_per_piece(size_t esize) { return (uint32_t)(16 / esize); }
VROD_TAG_HD inline uint32_t centroid_pieces(uint32_t dim, uint32_t per_piece) { return (dim + per_piece - 1) / per_piece; }
VROD_TAG_HD inline uint32_t centroid_team(uint32_t pieces) {
    uint32_t t = 1;
    while (t < pieces && t < kCentroidThreads) t *= 2;
    return t;
}
inline uint32_t centroid_groups(uint64_t count) { return row_pred_groups(count); }

}  // namespace vrod
