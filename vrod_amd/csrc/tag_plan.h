// tag_plan.h -- the host decisions of a tagged search (vrod_search_tagged): the batch's queries grouped by their
// predicate, and the narrow groups cut into scatter passes.  Plain arithmetic, no HIP headers (label_plan.h,
// search_plan.h): vrod_index.hip enqueues what these functions decide, tests/test_tag_plan.py compiles this header as
// host C++.  tag_matches is the one function the kernels share with the host (kernels_pred.hip).
//
// A narrow group (filter_route says its own rows are cheaper than a scan) gets a row list and is scored with the other
// narrow groups of its pass in the segmented launch of a labelled search (label_plan.h plan_segments).  A wide group
// takes the ordinary search flow over its mask: ONE SCAN PER DISTINCT WIDE PREDICATE, as one per wide label.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "label_plan.h"   // kNoSegment, PredGroups, group_preds

#if defined(__HIPCC__)
#define VROD_TAG_HD __host__ __device__
#else
#define VROD_TAG_HD
#endif

namespace vrod {

// One query's predicate over a row's 64 tag bits -- the layout of vrod_tag_pred (include/vrod.h): 24 bytes.
struct TagPred { uint64_t any, all, none; };
VROD_TAG_HD inline bool tag_matches(uint64_t t, uint64_t any, uint64_t all, uint64_t none) {
    return (any == 0 || (t & any) != 0) && (t & all) == all && (t & none) == 0;
}
// A bit both required and forbidden: no row can match, whatever its tags.
inline bool tag_unsatisfiable(const TagPred& p) { return (p.all & p.none) != 0; }

// Distinct predicates one pass over the tag array serves.  kernels_pred.hip keeps the predicate table (24 B) and one
// counter (4 B) per group in LDS: 2048 groups are 56 KiB, under the 64 KiB a launch gets without asking for more.
// (The pass asks for the LDS of the groups it has, so a small batch keeps the CU's occupancy.)
constexpr uint32_t kTagGroupsPerPass = 2048;
constexpr uint32_t kTagLdsPerGroup = 28;

// ------------------------------------------------------------------ grouping
// Tag predicates (label_plan.h group_preds): ordered by (any, all, none).
using TagGroups = PredGroups<TagPred>;
inline bool tag_before(const TagPred& a, const TagPred& b) {
    if (a.any != b.any) return a.any < b.any;
    if (a.all != b.all) return a.all < b.all;
    return a.none < b.none;
}
inline TagGroups tag_groups(const TagPred* p, uint32_t nq) { return group_preds(p, nq, tag_unsatisfiable, tag_before); }

// ------------------------------------------------------------------ scatter passes
// One pass over the tag array writes the row lists of the narrow groups among [g0, g1): group g's list starts at
// seg_off[g - g0] of the pass's list buffer (kNoSegment: a wide group, no list), list_n entries in all.
struct TagPass {
    uint32_t g0, g1;
    uint32_t n_lists;                // narrow groups among them (> 0)
    uint64_t list_n;
    std::vector<uint32_t> seg_off;   // [g1 - g0]
};
// m[g]: the group's matching eligible rows, narrow[g]: it takes a list.  A row sits in the list of every narrow group
// it matches, so the lists of a batch are not bounded by the corpus: passes of consecutive groups, cut where the next
// narrow group would take the pass's lists over `max_bytes` (the 1 GiB rule of the gather and exact paths) or the pass
// over `max_groups` groups (the LDS table).  A group whose own list exceeds max_bytes is served alone.  Every narrow
// group is in exactly one pass; a run of wide groups adds no pass of its own.  (Labels' groups are disjoint, their lists
// hold the corpus at the most: a labelled search passes no limit, kNoListLimit, and gets one pass per max_groups.)
constexpr uint64_t kNoListLimit = ~0ull;
inline std::vector<TagPass> plan_tag_passes(const std::vector<uint32_t>& m, const std::vector<uint8_t>& narrow,
                                            uint64_t max_bytes = 1ull << 30, uint32_t max_groups = kTagGroupsPerPass) {
    std::vector<TagPass> passes;
    const uint32_t G = (uint32_t)m.size();
    TagPass p{0, 0, 0, 0, {}};
    auto close = [&](uint32_t g) {
        if (p.n_lists) passes.push_back(p);
        p = TagPass{g, g, 0, 0, {}};
    };
    for (uint32_t g = 0; g < G; ++g) {
        if (g - p.g0 == max_groups || (narrow[g] && p.n_lists && (p.list_n + m[g]) * 4 > max_bytes)) close(g);
        p.seg_off.push_back(narrow[g] ? (uint32_t)p.list_n : kNoSegment);
        if (narrow[g]) { p.list_n += m[g]; p.n_lists++; }
        p.g1 = g + 1;
    }
    close(G);
    return passes;
}

}  // namespace vrod
