// aggregate_plan.h -- the arithmetic of row aggregation (vrod_index_aggregate_where): the key a row has in each mode, the
// home slots of the two hash tables and their sizes, the two orders of the result and the launch geometry.  Plain
// arithmetic, no HIP headers (rowpred_plan.h): vrod_index.hip enqueues what these functions decide, kernels_aggregate.hip
// calls the VROD_TAG_HD ones on the device, tests/test_aggregate_plan.py compiles this header as host C++.
//
// Both tables are open addressing with linear probing over a power of two of slots, claimed by one 64-bit
// compare-and-swap on the key word, so key and claim become visible together and nobody waits for a claimer.  Every
// int64 is a possible key (BY_VALUE with width 1), so no key value can mark an empty slot: the one key that equals the
// marker, kAggEmptyKey, never enters the hashed part -- it owns slot `slots`, one past the hashed ones, which needs no
// claim.  Whether ANY slot holds a group is read from its count (a group has at least one row), never from its key.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "keys_plan.h"     // key_hash
#include "rowpred_plan.h"   // kRowPredRowsPerGroup, row_pred_groups (and VROD_TAG_HD)

namespace vrod {

constexpr uint32_t kAggByLabel = 0, kAggByValue = 1, kAggByTag = 2;   // VROD_AGG_BY_*
constexpr uint32_t kAggOrderCount = 4;                                // VROD_AGG_ORDER_COUNT
constexpr uint32_t kAggMaxGroups = 1u << 20;                          // VROD_MAX_AGG_GROUPS
constexpr uint32_t kAggTagGroups = 64;                                // BY_TAG: a group per bit, directly indexed

// The layout of vrod_agg_group (include/vrod.h): 48 bytes, no padding.
struct AggGroup { int64_t key; uint64_t count; int64_t min_value, max_value, sum_value; uint64_t first_id; };
// What a slot holds before any row reached it: the identities of the five aggregates.
constexpr uint64_t kAggNoId = UINT64_MAX;
constexpr int64_t kAggEmptyKey = INT64_MIN;   // in a hashed slot's key word: not claimed yet

// floor(v / width) for width >= 1: C++ division truncates, so a negative v with a remainder goes one further down.
// Every result fits (|q| <= |v|), INT64_MIN / 1 included.
VROD_TAG_HD inline int64_t agg_floor_div(int64_t v, int64_t width) {
    if (width == 1) return v;
    const int64_t q = v / width;
    return (v % width != 0 && v < 0) ? q - 1 : q;
}
// The key of a row under BY_LABEL and BY_VALUE (BY_TAG has up to 64 keys per row: the indices of its set bits).
VROD_TAG_HD inline int64_t agg_key(uint32_t by, uint32_t label, int64_t value, int64_t width) {
    return by == kAggByLabel ? (int64_t)label : agg_floor_div(value, width);
}

// Home slots.  The global table takes the hash's low bits, a work-group's LDS table the bits from 32 up: keys that
// collide in one table are spread in the other, unless chosen to collide in both (tests/test_gpu_aggregate.py does).
VROD_TAG_HD inline uint64_t agg_home(int64_t key, uint64_t slots) { return key_hash((uint64_t)key) & (slots - 1); }
VROD_TAG_HD inline uint32_t agg_lds_home(int64_t key, uint32_t slots) { return (uint32_t)(key_hash((uint64_t)key) >> 32) & (slots - 1u); }

// The global table's hashed slots for a handle of `count` rows: a power of two, at least twice the groups a call can
// hold -- min(count, kAggMaxGroups) -- and at least kAggMinSlots.  So a call within the cap never fills more than half
// of it, and the largest table is 2^21 slots (+ the marker key's one) of 48 bytes.
constexpr uint64_t kAggMinSlots = 1024;
inline uint64_t agg_table_slots(uint64_t count) {
    const uint64_t n = count < kAggMaxGroups ? count : kAggMaxGroups;
    uint64_t s = kAggMinSlots;
    while (s < 2 * n) s *= 2;
    return s;
}
// A work-group's LDS table: kAggLdsSlots hashed slots (+ the marker key's one), six 8-byte words each: 24 KiB, six
// work-groups a CU.  A key that meets neither itself nor an empty slot within kAggLdsProbe steps of its home goes
// straight to the global table.
constexpr uint32_t kAggLdsSlots = 512;
constexpr uint32_t kAggLdsProbe = 8;
static_assert((kAggLdsSlots & (kAggLdsSlots - 1)) == 0 && (kAggLdsSlots + 1) * 48 <= 32 * 1024, "a power of two, within half of a plain launch's LDS");

// The device counters of one call, and the bits of `err` (the host reads the block once per pass).
struct AggCounters { uint64_t claimed, err, rows, n_out; };
constexpr uint64_t kAggErrGroups = 1;   // more than kAggMaxGroups hashed slots were claimed: VROD_ERR_CAPACITY
constexpr uint64_t kAggErrFull = 2;     // a probe ran over every slot: the sizing rule is broken, VROD_ERR_INTERNAL

// The global table as the kernels take it: a view into one block, [AggCounters | key | count | min | max | sum | first_id],
// each array slots + 1 words (the last slot is the marker key's; a BY_TAG table has kAggTagGroups directly indexed slots
// and leaves it unused).  Words apart, not structs: every atomic is one aligned 64-bit operation.
struct AggTable {
    AggCounters* ctr;
    int64_t* key;
    uint64_t* count;
    int64_t *min_value, *max_value;
    uint64_t *sum_value, *first_id;
    uint64_t slots;
};
inline size_t agg_table_bytes(uint64_t slots) { return sizeof(AggCounters) + (size_t)(slots + 1) * sizeof(AggGroup); }
inline AggTable agg_table_view(void* base, uint64_t slots) {
    AggTable t;
    const uint64_t n = slots + 1;
    t.ctr = (AggCounters*)base;
    t.key = (int64_t*)(t.ctr + 1);
    t.count = (uint64_t*)(t.key + n);
    t.min_value = (int64_t*)(t.count + n);
    t.max_value = t.min_value + n;
    t.sum_value = (uint64_t*)(t.max_value + n);
    t.first_id = t.sum_value + n;
    t.slots = slots;
    return t;
}

// The two orders of the result.  Keys are unique within a result, so both are total.
inline bool agg_before_key(const AggGroup& a, const AggGroup& b) { return a.key < b.key; }
inline bool agg_before_count(const AggGroup& a, const AggGroup& b) { return a.count != b.count ? a.count > b.count : a.key < b.key; }

// Launch geometry: the row-predicate passes' -- a work-group owns kRowPredRowsPerGroup rows, 64 rows a wave at a time.
constexpr uint32_t kAggThreads = kRowPredThreads;
inline uint32_t agg_groups(uint64_t count) { return row_pred_groups(count); }

}  // namespace vrod
