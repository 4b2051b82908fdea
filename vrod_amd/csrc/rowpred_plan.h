// rowpred_plan.h -- the host decisions of the row-predicate operations (vrod_index_count_where, _select_where,
// _delete_where, _set_filter_where, _set_tags_where).  Plain arithmetic, no HIP headers (where_plan.h, tag_plan.h):
// vrod_index.hip enqueues what these functions decide, tests/test_rowpred_plan.py compiles this header as host C++.
// row_pred_matches is the one function the kernels share with the host (kernels_pred.hip, kernels_rowpred.hip).
//
// The predicate is the one of vrod_search_where with the row's label beside it; here it is an operation on the rows
// themselves, not a restriction of one search.
#pragma once
#include <stdint.h>

#include "where_plan.h"   // where_matches (and VROD_TAG_HD)

namespace vrod {

// The layout of vrod_row_pred (include/vrod.h): 48 bytes, no padding.
struct RowPred { uint64_t any, all, none; int64_t lo, hi; uint32_t label, has_label; };
// A row with tags t, value v and label l.  The label is compared only when the predicate carries one.
VROD_TAG_HD inline bool row_pred_matches(uint64_t t, int64_t v, uint32_t l, const RowPred& p) {
    return where_matches(t, v, p.any, p.all, p.none, p.lo, p.hi) && (!p.has_label || l == p.label);
}
// bit r of `scope` set = row r is out of scope (deleted, or not allowed); null: every row below count is in scope
VROD_TAG_HD inline bool row_in_scope(const uint32_t* scope, uint64_t r, uint64_t count) {
    return r < count && !(scope && ((scope[r >> 5] >> (r & 31u)) & 1u));
}
// An empty interval, or a bit both required and forbidden: no row can match, whatever it carries (every label can occur).
inline bool row_pred_unsatisfiable(const RowPred& p) { return p.lo > p.hi || (p.all & p.none) != 0; }
// Identical predicates are counted once: the order of the table one pass serves (has_label is 0 or 1 by then).
inline bool row_pred_before(const RowPred& a, const RowPred& b) {
    if (a.any != b.any) return a.any < b.any;
    if (a.all != b.all) return a.all < b.all;
    if (a.none != b.none) return a.none < b.none;
    if (a.lo != b.lo) return a.lo < b.lo;
    if (a.hi != b.hi) return a.hi < b.hi;
    if (a.has_label != b.has_label) return a.has_label < b.has_label;
    return a.has_label && a.label < b.label;
}

// Distinct predicates one pass of vrod_index_count_where over the three columns serves.  kernels_pred.hip keeps the table
// (48 B) and one counter (4 B) per predicate in LDS: 1024 predicates are 52 KiB, under the 64 KiB a launch gets without
// asking for more, as where_plan.h chooses kWhereGroupsPerPass.  (The pass asks for the LDS of the predicates it has.)
constexpr uint32_t kRowPredsPerPass = 1024;
constexpr uint32_t kRowPredLdsPerPred = 52;

// Rows one work-group owns in every pass: 32 whole 64-row waves, and exactly the 64 words of the hit bitmap one wave
// reads back -- a lane a word -- when it scatters a selection.  Per-work-group counts and a prefix over them give every
// group's first output position, so no atomic decides an order or a count.
constexpr uint32_t kRowPredRowsPerGroup = 2048;
constexpr uint32_t kRowPredThreads = 256;   // of the single-predicate passes: 4 waves, 8 rows a lane
static_assert(kRowPredRowsPerGroup % 64 == 0 && kRowPredRowsPerGroup / 32 == 64, "whole waves; a hit word per lane of the scatter's wave");
static_assert(kRowPredRowsPerGroup % kRowPredThreads == 0, "every lane walks the same number of rows");
inline uint32_t row_pred_groups(uint64_t count) { return (uint32_t)((count + kRowPredRowsPerGroup - 1) / kRowPredRowsPerGroup); }
// 32-bit words of the hit bitmap the passes write for `count` rows: whole waves, so lanes 0 and 32 never test a bound
inline uint64_t row_pred_hit_words(uint64_t count) { return (count + 63) / 64 * 2; }

}  // namespace vrod
