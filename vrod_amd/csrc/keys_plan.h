// keys_plan.h -- the host side of the row keys (vrod_index_set_keys, vrod_index_find_keys, ...; vrod_index.hip): the
// hash, the home slot and the sizing rule of the device key table (kernels_keys.hip, DESIGN.md "Row keys").  Plain
// host-and-device functions, no HIP runtime call: tests/test_keys_plan.py compiles this header as host C++.
//
// The table is open addressing with linear probing over `slots` entries (a power of two, at least kKeyMinSlots):
// slot_key[slots] u64 (kKeyNone = empty) and slot_row[slots] u32.  A slot is never emptied again; what makes a found
// slot an answer is the key column (key_column[slot_row] == key and the row live), so slots left behind by deletes and
// re-keying are harmless and only cost load.  The load rule keeps the occupied slots, stale ones included, at or below
// half the table, which also bounds every walk: an empty slot is always met.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VROD_KEYS_HD __host__ __device__
#else
#define VROD_KEYS_HD
#endif

namespace vrod {

constexpr uint64_t kKeyNone = UINT64_MAX;      // VROD_ID_NONE: "no key", and an empty slot
constexpr uint64_t kKeyMinSlots = 1024;
// words of the table's device counters (KeyCounters, kernels_keys.hip)
constexpr uint32_t kKeyErrFull = 1u;           // a probe loop ran over every slot without an end: VROD_ERR_INTERNAL
constexpr uint32_t kKeyErrHeld = 2u;           // check: a key is held by a live row outside the range; rebuild: by two live rows

// the snapshot checksum's mixer (snapshot_plan.h snap_mix) over key + golden: all arithmetic mod 2^64
VROD_KEYS_HD inline uint64_t key_hash(uint64_t key) {
    uint64_t z = key + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
VROD_KEYS_HD inline uint64_t key_home(uint64_t key, uint64_t slots) { return key_hash(key) & (slots - 1); }

// Slots of a table built for n keys (the live keyed rows plus the incoming ones) that has `cur` slots now (0: none
// yet): doubled from max(cur, kKeyMinSlots) until n fits in a quarter of it.  A table never shrinks.
inline uint64_t key_table_slots(uint64_t n, uint64_t cur) {
    uint64_t s = cur > kKeyMinSlots ? cur : kKeyMinSlots;
    while (n > s / 4) s *= 2;
    return s;
}
// An insert of `incoming` keys into a table with `occupied` slots in use (stale ones included) could cross the load
// limit of one half (every incoming key may claim a new slot): rebuild first.
inline bool key_needs_rebuild(uint64_t occupied, uint64_t incoming, uint64_t slots) { return occupied + incoming > slots / 2; }

}  // namespace vrod
