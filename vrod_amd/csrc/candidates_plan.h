// candidates_plan.h -- the host decisions of the candidate-list searches (vrod_search_candidates, vrod_score_candidates):
// whether a lims array is one and no list is too long, the sort network and the work-group a list's length asks for, the
// slot tables the segmented driver gets once the lists are resolved, and the tiles of the ragged score launch.  Plain
// arithmetic, no HIP headers (combine_plan.h, label_plan.h): vrod_index.hip enqueues what these functions decide,
// tests/test_candidates_plan.py compiles this header as host C++.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "label_plan.h"   // SlotTables

namespace vrod {

// List entries per query (VROD_MAX_CANDIDATES, include/vrod.h): one list, as 32-bit rows, fills the 64 KB of LDS the
// sort's work-group holds it in (kernels_candidates.hip).
constexpr uint32_t kCandMaxList = 16384;
// A list entry that names no eligible row, after cand_resolve.
constexpr uint32_t kCandNoRow = 0xFFFFFFFFu;

// The lims array.  0: fine; 1: it does not start at 0, or it decreases; 2: query *bad_q lists more than kCandMaxList ids.
inline int cand_check_lims(const uint32_t* lims, uint32_t nq, uint32_t* bad_q) {
    if (lims[0] != 0) return 1;
    for (uint32_t q = 0; q < nq; ++q)
        if (lims[q + 1] < lims[q]) return 1;
    for (uint32_t q = 0; q < nq; ++q)
        if (lims[q + 1] - lims[q] > kCandMaxList) { *bad_q = q; return 2; }
    return 0;
}

// Entries of the bitonic network that sorts a list of `len`: the next power of two (a list of 0 or 1 needs no stage).
inline uint32_t cand_network_size(uint32_t len) {
    uint32_t p = len ? 1u : 0u;
    while (p < len) p <<= 1;
    return p;
}

// The sort launches of a batch: a query goes to the smallest class whose capacity holds its network, and each class
// with a query in it is one launch of work-groups of its own size and LDS (capacity x 4 B), one work-group per query.
// Within its work-group a query still runs the network of its own length only.
constexpr uint32_t kCandClasses = 3;
constexpr uint32_t kCandClassCap[kCandClasses] = {256, 4096, kCandMaxList};
constexpr uint32_t kCandClassThreads[kCandClasses] = {64, 256, 1024};
inline uint32_t cand_sort_class(uint32_t len) {
    const uint32_t n = cand_network_size(len);
    uint32_t c = 0;
    while (n > kCandClassCap[c]) ++c;
    return c;
}
// The batch's queries ordered by class, ascending within a class: class c owns order[first[c] .. first[c + 1]).
struct CandSortPlan {
    std::vector<uint32_t> order;
    uint32_t first[kCandClasses + 1] = {};
};
inline CandSortPlan cand_sort_plan(const uint32_t* lims, uint32_t nq) {
    CandSortPlan P;
    P.order.resize(nq);
    uint32_t n[kCandClasses] = {};
    for (uint32_t q = 0; q < nq; ++q) n[cand_sort_class(lims[q + 1] - lims[q])]++;
    for (uint32_t c = 0; c < kCandClasses; ++c) P.first[c + 1] = P.first[c] + n[c];
    uint32_t at[kCandClasses];
    std::copy(P.first, P.first + kCandClasses, at);
    for (uint32_t q = 0; q < nq; ++q) P.order[at[cand_sort_class(lims[q + 1] - lims[q])]++] = q;
    return P;
}

// The segmented driver's tables for the resolved lists: query q's len[q] distinct eligible rows lie ascending in the list
// buffer from lims[q] on, so every query with a row is one group of one slot (slot_q = q, slot_len = len[q], slot_base =
// lims[q]).  The queries without a row get no slot: their result rows are filled as unfilled, n_empty of them.
struct CandSlots {
    SlotTables T;
    uint32_t n_empty = 0, max_len = 0;
    uint64_t rows = 0;   // sum of the lengths: the rows the search scores
};
inline CandSlots cand_slot_tables(const uint32_t* lims, const uint32_t* len, uint32_t nq) {
    CandSlots S;
    for (uint32_t q = 0; q < nq; ++q) {
        if (!len[q]) { S.n_empty++; continue; }
        S.T.add(lims[q], len[q], &q, 1);
        S.max_len = std::max(S.max_len, len[q]);
        S.rows += len[q];
    }
    return S;
}

// The ragged score launch (vrod_score_candidates): one wave per tile of 64 consecutive entries of one query's list, the
// tiles of query q being blocks [off[q], off[q + 1]) of the launch.  cand_tile_query is shared with the kernel.
inline std::vector<uint32_t> cand_tile_offsets(const uint32_t* lims, uint32_t nq) {
    std::vector<uint32_t> off((size_t)nq + 1, 0u);
    for (uint32_t q = 0; q < nq; ++q) off[q + 1] = off[q] + (lims[q + 1] - lims[q] + 63) / 64;
    return off;
}
VROD_LABEL_HD inline uint32_t cand_tile_query(const uint32_t* off, uint32_t nq, uint32_t b) {
    uint32_t lo = 0, hi = nq;   // off[lo] <= b < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (off[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace vrod
