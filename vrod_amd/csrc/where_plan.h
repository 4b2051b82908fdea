// where_plan.h -- the host decisions of a search with a tags + value-interval predicate per query (vrod_search_where).
// Plain arithmetic, no HIP headers (tag_plan.h, label_plan.h): vrod_index.hip enqueues what these functions decide,
// tests/test_where_plan.py compiles this header as host C++.  where_matches is the one function the kernels share with
// the host (kernels_pred.hip).
//
// The search is the tagged search with a wider predicate: the same grouping (label_plan.h group_preds), the same scatter
// passes (plan_tag_passes) and the same routing; only the predicate, its order and the groups one pass serves differ.
#pragma once
#include <stdint.h>

#include "tag_plan.h"   // tag_matches, group_preds, plan_tag_passes, kNoSegment

namespace vrod {

// One query's predicate over a row's 64 tag bits and its signed 64-bit value -- the layout of vrod_where
// (include/vrod.h): 40 bytes.
struct WherePred { uint64_t any, all, none; int64_t lo, hi; };
// Signed compare, both ends inclusive.
VROD_TAG_HD inline bool where_matches(uint64_t t, int64_t v, uint64_t any, uint64_t all, uint64_t none, int64_t lo, int64_t hi) {
    return tag_matches(t, any, all, none) && lo <= v && v <= hi;
}
// An empty interval, or a bit both required and forbidden: no row can match, whatever it carries.
inline bool where_unsatisfiable(const WherePred& p) { return p.lo > p.hi || (p.all & p.none) != 0; }

// Distinct predicates one pass over the tag and value arrays serves.  kernels_pred.hip keeps the predicate table
// (40 B) and one counter (4 B) per group in LDS: 1024 groups are 44 KiB, under the 64 KiB a launch gets without asking
// for more.  (The pass asks for the LDS of the groups it has.)
constexpr uint32_t kWhereGroupsPerPass = 1024;
constexpr uint32_t kWhereLdsPerGroup = 44;

// The batch's distinct satisfiable predicates ordered by (any, all, none, lo, hi), the interval ends as signed values.
using WhereGroups = PredGroups<WherePred>;
inline bool where_before(const WherePred& a, const WherePred& b) {
    if (a.any != b.any) return a.any < b.any;
    if (a.all != b.all) return a.all < b.all;
    if (a.none != b.none) return a.none < b.none;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.hi < b.hi;
}
inline WhereGroups where_groups(const WherePred* p, uint32_t nq) { return group_preds(p, nq, where_unsatisfiable, where_before); }

}  // namespace vrod
