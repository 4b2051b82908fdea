// group_plan.h -- the host decisions of a grouped search (vrod_search_grouped): how many results the first-stage search
// asks for, when a query's de-duplicated list is final, and the sizes of the de-duplication kernel's LDS tables.  Plain
// arithmetic, no HIP headers (search_plan.h, label_plan.h): vrod_index.hip enqueues what these functions decide,
// tests/test_group_plan.py compiles this header as host C++.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace vrod {

// The largest k of the ABI (VROD_MAX_K, include/vrod.h; = kSelectChunk / 2 - 512, so a list of this length always passes
// through the select chain).
constexpr uint32_t kGroupMaxK = 3584;

// Results per query the candidate search asks for: enough that k distinct labels are usually among them -- four times
// k, and at least 32 more than k so that k = 1 does not go to the dense stage over one duplicate -- but never more than
// the ABI's largest k or the eligible rows (a list as long as the eligible rows holds them all).  0 without an
// eligible row.
inline uint32_t group_first_k(uint32_t k, uint64_t eligible) {
    const uint64_t rule = std::max<uint64_t>(4ull * k, (uint64_t)k + 32);
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(kGroupMaxK, eligible), rule);
}

// A query is resolved -- its first min(k, found) distinct labels are final -- once it has k of them, or once the list it
// was de-duplicated from held every row that could still add a label: the list came back short (`valid` < k1 real
// entries), or it was as long as the eligible rows.  Until then the rows below the list's last entry are unknown.
inline bool group_resolved(uint32_t found, uint32_t k, uint32_t valid, uint32_t k1, uint64_t eligible) {
    return found >= k || valid < k1 || k1 >= eligible;
}

// De-duplication kernel (kernels_group.hip): one work-group per query holds the labels taken so far (fewer than k) and
// the labels of the k1 candidates in LDS, and a hash table over them of a power of two of slots, at least twice the
// entries while that fits 64 KB beside them (the worst case, 3583 + 3584 entries in 8192 slots, still has empty slots).
constexpr uint32_t kGroupDedupeMaxSlots = 8192;
inline uint32_t group_dedupe_entries(uint32_t k, uint32_t k1) { return k - 1 + k1; }
inline uint32_t group_dedupe_slots(uint32_t k, uint32_t k1) {
    uint32_t s = 64;
    while (s < 2 * group_dedupe_entries(k, k1) && s < kGroupDedupeMaxSlots) s <<= 1;
    return s;
}

// Rows per work-group of the dense stage's mask pass: whole 256-row wave steps, each work-group builds the hash set of
// its query's taken labels once.
constexpr uint32_t kGroupMaskRowsPerBlock = 16384;

}  // namespace vrod
