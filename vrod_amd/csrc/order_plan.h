// order_plan.h -- the arithmetic of ordered selection (vrod_index_select_ordered): the key a value becomes, the cursor
// test, the radix select's bucket choice and the launch geometry.  Plain arithmetic, no HIP headers (rowpred_plan.h):
// vrod_index.hip enqueues what these functions decide, kernels_order.hip calls the VROD_TAG_HD ones on the device,
// tests/test_order_plan.py compiles this header as host C++.
//
// The order of a call is (value, id) ascending, or value descending and id STILL ascending.  A row's key is its value
// mapped so that unsigned key order is the call's value order; (key, id) ascending as a pair of unsigned 64-bit words
// is then the call's order in both directions, and every pass compares nothing else.
#pragma once
#include <stdint.h>

#include "rowpred_plan.h"   // kRowPredRowsPerGroup, row_pred_groups (and VROD_TAG_HD)

namespace vrod {

// Signed order as unsigned order (the sign bit flipped); complemented under DESC, which reverses it.
VROD_TAG_HD inline uint64_t order_key(int64_t v, bool desc) {
    const uint64_t k = (uint64_t)v ^ (1ull << 63);
    return desc ? ~k : k;
}
// ... and back: the value a key came from
VROD_TAG_HD inline int64_t order_value(uint64_t key, bool desc) { return (int64_t)((desc ? ~key : key) ^ (1ull << 63)); }
// Is (key, id) strictly after the cursor (ckey, cid)?  The cursor need not name a row.
VROD_TAG_HD inline bool order_after(uint64_t key, uint64_t id, uint64_t ckey, uint64_t cid) {
    return key > ckey || (key == ckey && id > cid);
}

// The radix select walks the key from its most significant byte down: round i looks at bits [56 - 8i, 64 - 8i).
constexpr uint32_t kOrderRounds = 8;
constexpr uint32_t kOrderBins = 256;
VROD_TAG_HD inline uint32_t order_digit(uint64_t key, uint32_t round) { return (uint32_t)(key >> (56u - 8u * round)) & 255u; }
// Do the digits of `key` above round `round` equal those of `prefix`?  (Round 0 has none above it.)
VROD_TAG_HD inline bool order_in_prefix(uint64_t key, uint64_t prefix, uint32_t round) {
    return round == 0u || ((key ^ prefix) >> (64u - 8u * round)) == 0ull;
}
// The bucket that holds the element of rank `remaining` (1-based, 1 <= remaining <= the histogram's sum) among the keys
// a histogram counts, and the rank left inside that bucket: remaining minus everything in the buckets before it.
struct OrderPick { uint32_t digit, remaining; };
VROD_TAG_HD inline OrderPick order_pick(const uint32_t* hist, uint32_t remaining) {
    uint32_t d = 0;
    while (d + 1 < kOrderBins && hist[d] < remaining) remaining -= hist[d++];
    return OrderPick{d, remaining};
}

// What the select leaves on the device for the collect pass: every hit row with key < pivot is taken, and the first
// `remaining` hit rows, by ascending id, with key == pivot.  While the rounds run, pivot holds the digits chosen so far.
struct OrderState { uint64_t pivot; uint32_t remaining, pad_; };

// Launch geometry: the row-predicate passes' -- a work-group owns kRowPredRowsPerGroup rows, the 64 hit words one wave
// reads back, 64 rows a wave at a time.
constexpr uint32_t kOrderThreads = kRowPredThreads;
constexpr uint32_t kOrderChunksPerGroup = kRowPredRowsPerGroup / 64;   // 64-row chunks a group walks: one ballot each
inline uint32_t order_groups(uint64_t count) { return row_pred_groups(count); }

// The sort: (key, id) records, padded to a power of two with records that sort after every real one (no row has the id
// UINT64_MAX: it is VROD_ID_NONE).  Up to kOrderSortTile records are sorted in one work-group's LDS (16 B each: 32 KiB);
// above that the bitonic network's steps at distances >= kOrderSortTile run in global memory, the rest of each merge in LDS.
constexpr uint32_t kOrderMaxRows = 65536;   // VROD_MAX_ORDERED
constexpr uint32_t kOrderSortTile = 2048;
constexpr uint32_t kOrderSortThreads = 256;
inline uint32_t order_sort_size(uint32_t n) {
    uint32_t p = kOrderSortTile;
    while (p < n) p <<= 1;
    return p;
}
// Bitonic network, element i at step (k, j), i's partner being i ^ j with i < (i ^ j): is the pair kept ascending?
VROD_TAG_HD inline bool order_bitonic_up(uint32_t i, uint32_t k) { return (i & k) == 0u; }

}  // namespace vrod
