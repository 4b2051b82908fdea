// kernels_keys.hip -- the device side of the row keys (gfx950): the key table of keys_plan.h and the gather that turns
// ids into keys.  Five kernels, each one thread per item with a grid-stride loop:
//   check      read-only: raises kKeyErrHeld when a key that a call gives to a live row of its range is held by a live
//              row outside the range (vrod_index_set_keys, before anything is written);
//   insert     the keys of the live rows [r0, r0 + n) of the key column go into the table; a key that has a slot
//              already gets that slot's row overwritten;
//   rebuild    the same walk over the whole column into a table that starts empty: there a key met again is held by two
//              live rows, which raises kKeyErrHeld (vrod_index_load: VROD_ERR_CORRUPT);
//   find       keys -> ids of the live rows that hold them;
//   translate  ids -> the keys their rows store (a gather over the key column, no table involved).
// These are latency-bound random accesses: one 8-byte load per slot visited, no reuse, nothing to tile.  A slot is
// claimed by one 64-bit atomicCAS on slot_key (a plain vector atomic); keys are unique among the live rows of a launch,
// so a slot's row has one writer per launch.  EVERY probe loop is bounded by `slots`: a walk that runs out raises
// kKeyErrFull and ends, it never spins -- the load rule (keys_plan.h) means it cannot happen on a sound table, and a
// table that is not sound must not hang the device.
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "keys_plan.h"

namespace vrod {

__device__ inline bool key_row_dead(const uint32_t* __restrict__ del, uint64_t r) { return del && ((del[r >> 5] >> (r & 31)) & 1u); }

// a 64-lane sum, then one atomic per wave
__device__ inline void key_wave_add(unsigned long long v, unsigned long long* dst) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}
__device__ inline void key_wave_max(uint32_t v, uint32_t* dst) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, v);
}

// The slot that holds `key`, or UINT64_MAX when an empty slot ends the walk (or the walk runs out: *full is set).
// *walk: slots visited.
__device__ inline uint64_t key_lookup(const KeyTable& T, uint64_t key, uint32_t* walk, bool* full) {
    const uint64_t mask = T.slots - 1;
    uint64_t s = key_home(key, T.slots);
    for (uint64_t p = 0; p < T.slots; ++p, s = (s + 1) & mask) {
        const uint64_t cur = T.slot_key[s];
        if (cur == key) { *walk = (uint32_t)(p + 1); return s; }
        if (cur == kKeyNone) { *walk = (uint32_t)(p + 1); return UINT64_MAX; }
    }
    *walk = (uint32_t)T.slots;
    *full = true;
    return UINT64_MAX;
}

// the live row < count that holds `key` according to the table and the key column, or UINT64_MAX
__device__ inline uint64_t key_holder(const KeyTable& T, const uint64_t* __restrict__ col, const uint32_t* __restrict__ del, uint64_t count,
                                      uint64_t key, uint32_t* walk, bool* full) {
    const uint64_t s = key_lookup(T, key, walk, full);
    if (s == UINT64_MAX) return UINT64_MAX;
    const uint64_t r = T.slot_row[s];
    if (r >= count || col[r] != key || key_row_dead(del, r)) return UINT64_MAX;   // a stale slot
    return r;
}

__global__ __launch_bounds__(256) void keys_check_kernel(KeyTable T, const uint64_t* __restrict__ col, const uint32_t* __restrict__ del,
                                                         uint64_t count, const uint64_t* __restrict__ keys, uint64_t r0, uint64_t n,
                                                         KeyCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t err = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        if (key == kKeyNone || key_row_dead(del, r0 + i)) continue;   // (deleted rows take no part in uniqueness)
        uint32_t walk = 0;
        bool full = false;
        const uint64_t r = key_holder(T, col, del, count, key, &walk, &full);
        if (full) err |= kKeyErrFull;
        if (r != UINT64_MAX && (r < r0 || r >= r0 + n)) err |= kKeyErrHeld;
    }
    if (err) atomicOr(&ctr->err, err);
}

// REBUILD: the table was empty when the launch began.
template <bool REBUILD>
__global__ __launch_bounds__(256) void keys_insert_kernel(KeyTable T, const uint64_t* __restrict__ col, const uint32_t* __restrict__ del,
                                                          uint64_t r0, uint64_t n, KeyCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, mask = T.slots - 1;
    const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long claimed = 0;
    uint32_t longest = 0, err = 0;
    for (uint64_t i = first; i < n; i += stride) {
        const uint64_t r = r0 + i, key = col[r];
        if (key == kKeyNone || key_row_dead(del, r)) continue;
        uint64_t s = key_home(key, T.slots);
        uint64_t p = 0;
        for (; p < T.slots; ++p, s = (s + 1) & mask) {
            uint64_t cur = T.slot_key[s];
            if (cur == kKeyNone) {
                cur = atomicCAS((unsigned long long*)&T.slot_key[s], (unsigned long long)kKeyNone, (unsigned long long)key);
                if (cur == kKeyNone) { ++claimed; T.slot_row[s] = (uint32_t)r; break; }
            }
            if (cur == key) {   // the key has a slot: it names this row from now on
                if (REBUILD) err |= kKeyErrHeld;
                T.slot_row[s] = (uint32_t)r;
                break;
            }
        }
        if (p == T.slots) err |= kKeyErrFull;
        longest = max(longest, (uint32_t)min(p + 1, T.slots));
    }
    key_wave_add(claimed, &ctr->claimed);
    key_wave_max(longest, &ctr->max_probe);
    if (err) atomicOr(&ctr->err, err);
}

__global__ __launch_bounds__(256) void keys_find_kernel(KeyTable T, const uint64_t* __restrict__ col, const uint32_t* __restrict__ del,
                                                        uint64_t count, uint64_t id_offset, const uint64_t* __restrict__ keys, uint64_t n,
                                                        uint64_t* __restrict__ out_ids, KeyCounters* __restrict__ ctr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long walked = 0;
    uint32_t err = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t key = keys[i];
        uint64_t id = kKeyNone;
        if (key != kKeyNone) {
            uint32_t walk = 0;
            bool full = false;
            const uint64_t r = key_holder(T, col, del, count, key, &walk, &full);
            if (full) err |= kKeyErrFull;
            if (r != UINT64_MAX) id = r + id_offset;
            walked += walk;
        }
        out_ids[i] = id;
    }
    key_wave_add(walked, &ctr->find_walk);
    if (err) atomicOr(&ctr->err, err);
}

__global__ __launch_bounds__(256) void keys_translate_kernel(const uint64_t* __restrict__ col, uint64_t count, uint64_t id_offset,
                                                             const uint64_t* __restrict__ ids, uint64_t n, uint64_t* __restrict__ out_keys) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t id = ids[i];
        uint64_t key = kKeyNone;
        if (id != kKeyNone && id >= id_offset && id - id_offset < count) key = col[id - id_offset];
        out_keys[i] = key;
    }
}

// ------------------------------------------------------------------ launchers
// latency-bound walks: enough work-groups to fill the device several times over, the rest by the grid-stride loops
static inline unsigned keys_grid(uint64_t items) { return (unsigned)std::min<uint64_t>(8192, std::max<uint64_t>(1, (items + 255) / 256)); }

void launch_keys_check(const KeyTable& T, const uint64_t* d_col, const uint32_t* d_del, uint64_t count, const uint64_t* d_keys, uint64_t r0,
                       uint64_t n, KeyCounters* d_ctr, hipStream_t s) {
    if (!n) return;
    keys_check_kernel<<<keys_grid(n), 256, 0, s>>>(T, d_col, d_del, count, d_keys, r0, n, d_ctr);
}

void launch_keys_insert(const KeyTable& T, const uint64_t* d_col, const uint32_t* d_del, uint64_t r0, uint64_t n, bool rebuild,
                        KeyCounters* d_ctr, hipStream_t s) {
    if (!n) return;
    if (rebuild) keys_insert_kernel<true><<<keys_grid(n), 256, 0, s>>>(T, d_col, d_del, r0, n, d_ctr);
    else keys_insert_kernel<false><<<keys_grid(n), 256, 0, s>>>(T, d_col, d_del, r0, n, d_ctr);
}

void launch_keys_find(const KeyTable& T, const uint64_t* d_col, const uint32_t* d_del, uint64_t count, uint64_t id_offset,
                      const uint64_t* d_keys, uint64_t n, uint64_t* d_out_ids, KeyCounters* d_ctr, hipStream_t s) {
    if (!n) return;
    keys_find_kernel<<<keys_grid(n), 256, 0, s>>>(T, d_col, d_del, count, id_offset, d_keys, n, d_out_ids, d_ctr);
}

void launch_keys_translate(const uint64_t* d_col, uint64_t count, uint64_t id_offset, const uint64_t* d_ids, uint64_t n, uint64_t* d_out_keys,
                           hipStream_t s) {
    if (!n) return;
    keys_translate_kernel<<<keys_grid(n), 256, 0, s>>>(d_col, count, id_offset, d_ids, n, d_out_keys);
}

}  // namespace vrod
