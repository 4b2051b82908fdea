// combine_plan.h -- the host decisions of a search by weighted examples (vrod_search_combined): whether a lims array is
// one, how many terms and excluded ids each query and the batch carry, how many results the underlying search asks for,
// and the limits on all of them.  Plain arithmetic, no HIP headers (byid_plan.h, search_plan.h): vrod_index.hip enqueues
// what these functions decide, tests/test_combine_plan.py compiles this header as host C++.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace vrod {

// The limits of the ABI (VROD_MAX_COMBINE_TERMS, VROD_MAX_EXCLUDE, VROD_MAX_K, VROD_COMBINED_EXCLUDE_TERMS; include/vrod.h).
constexpr uint32_t kCombineMaxTerms = 256, kCombineMaxExclude = 1024, kCombineMaxK = 3584;
constexpr uint32_t kCombineExcludeTerms = 1u;

// nq + 1 entries that start at 0 and never decrease: query q owns [lims[q], lims[q + 1]).
inline bool combine_lims_ok(const uint32_t* lims, uint32_t nq) {
    if (lims[0] != 0) return false;
    for (uint32_t q = 0; q < nq; ++q)
        if (lims[q + 1] < lims[q]) return false;
    return true;
}

// Query q's terms, and its excluded entries: its exclude list (excl_lims may be null: none) plus, under the flag, its
// terms -- duplicates counted, since the drop launch holds them all.  64 bits: two uint32 differences may sum past 2^32.
inline uint32_t combine_terms(const uint32_t* term_lims, uint32_t q) { return term_lims[q + 1] - term_lims[q]; }
inline uint64_t combine_excluded(const uint32_t* term_lims, const uint32_t* excl_lims, uint32_t q, bool exclude_terms) {
    return (uint64_t)(excl_lims ? excl_lims[q + 1] - excl_lims[q] : 0u) + (exclude_terms ? combine_terms(term_lims, q) : 0u);
}

// Results per query of the underlying search: the top k of S \ X is the first k of the top (k + |X|) of S with X removed,
// and one k1 serves the batch -- the largest excluded count decides.
inline uint32_t combine_search_k(uint32_t k, uint32_t max_excluded) { return k + max_excluded; }

// What the arguments alone decide.  0: fine, 1: unknown flag bits, 2: k out of 1..kCombineMaxK.
inline int combine_check_args(uint32_t k, uint32_t flags) {
    if (flags & ~kCombineExcludeTerms) return 1;
    if (k < 1 || k > kCombineMaxK) return 2;
    return 0;
}

// The batch.  0: fine, else the first failure: 3 term_lims is no lims array, 4 excl_lims is none, 5 a query without an
// operand (no vector and no term), 6 a query with more than kCombineMaxTerms terms, 7 one with more than
// kCombineMaxExclude excluded entries, 8 k + the largest excluded count is past kCombineMaxK.  *bad_q: the query of
// failures 5 .. 7.  Filled on success: the batch's largest term count and largest excluded count.
struct CombineCounts { uint32_t max_terms = 0, max_excluded = 0; };
inline int combine_check_batch(const uint32_t* term_lims, const uint32_t* excl_lims, uint32_t nq, bool has_vector, uint32_t k, uint32_t flags,
                               CombineCounts* out, uint32_t* bad_q) {
    const bool ex = flags & kCombineExcludeTerms;
    if (!combine_lims_ok(term_lims, nq)) return 3;
    if (excl_lims && !combine_lims_ok(excl_lims, nq)) return 4;
    CombineCounts c;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t t = combine_terms(term_lims, q);
        const uint64_t x = combine_excluded(term_lims, excl_lims, q, ex);
        *bad_q = q;
        if (!has_vector && t == 0) return 5;
        if (t > kCombineMaxTerms) return 6;
        if (x > kCombineMaxExclude) return 7;
        c.max_terms = std::max(c.max_terms, t);
        c.max_excluded = std::max(c.max_excluded, (uint32_t)x);
    }
    if (combine_search_k(k, c.max_excluded) > kCombineMaxK) return 8;
    *out = c;
    return 0;
}

// Lanes that own one query in the combine launch: a wave while every lane holds at most four 16-B units of the stored
// row, the whole work-group for longer rows.
inline uint32_t combine_lanes_per_query(uint32_t dim, uint32_t elem_bytes) {
    const uint32_t units = (dim * elem_bytes + 15) / 16;
    return units <= 256 ? 64u : 256u;
}

}  // namespace vrod
