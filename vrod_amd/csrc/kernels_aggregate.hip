// kernels_aggregate.hip -- the device side of row aggregation (vrod_index_aggregate_where; gfx950): count, min, max and
// sum of the value and the smallest id of every group of the rows a row predicate matches, the groups being the rows'
// labels, value buckets or tag bits.  Exact and deterministic.
//
// The reference has no attributes beside a row (src/database/mod.rs), so it has nothing to group by; "how many chunks
// does each tenant hold" needs the GROUP BY of the row-predicate family.
//
// The keys are not known in advance, so positions cannot come from prefix sums as in every other column pass: this is
// a hash aggregation, and the only pass of the library whose results go through atomics.  All five aggregates are
// commutative integer operations (add mod 2^64, signed min / max, unsigned min), so the order the atomics land in
// changes no bit of the result.  Three launches over the geometry of kernels_rowpred.hip (work-group b owns rows
// [b * R, (b + 1) * R), R = kRowPredRowsPerGroup, a wave covers 64 rows at a time):
//   reset   : every slot of the global table to the identities, its key word to "empty" -- BEFORE the pass, so that a
//             lane that finds a key an instant after its claimer never adds into a slot the claimer is still preparing;
//   pass    : three levels.  A wave whose matching rows all share one key folds them with shuffles and spends one set
//             of atomics on the lot (a corpus under one label is this case everywhere); otherwise a lane a row.  Either
//             way the rows go into the work-group's LDS table first (aggregate_plan.h: open addressing, a probe of at
//             most kAggLdsProbe steps, 64-bit LDS atomics at work-group scope), and a key that finds no LDS slot goes
//             straight to the global table.  At the end every occupied LDS slot is merged into the global table with
//             agent-scope atomics: one global insert per (work-group, distinct key), not per row.  BY_TAG has 64
//             directly indexed slots at both levels and folds the rows of each bit a wave carries;
//   compact : the occupied global slots as dense vrod_agg_group records, positions from an atomic counter -- the host
//             orders them afterwards, so the positions decide nothing.
// No atomic returns a value except the claims (a compare-and-swap, and the claim counter that enforces the group cap).
#include "aggregate_plan.h"
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

#define AGG_RLX __ATOMIC_RELAXED
#define AGG_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define AGG_DEV __HIP_MEMORY_SCOPE_AGENT

// What some rows of one key add up to.
struct AggPart { uint64_t count; int64_t mn, mx; uint64_t sum, first; };

// The LDS table: the global table's six arrays, kAggLdsSlots hashed slots and the marker key's.
struct AggLds {
    long long key[kAggLdsSlots + 1];
    unsigned long long count[kAggLdsSlots + 1];
    long long mn[kAggLdsSlots + 1], mx[kAggLdsSlots + 1];
    unsigned long long sum[kAggLdsSlots + 1], first[kAggLdsSlots + 1];
};
constexpr uint32_t kAggNoLdsSlot = UINT32_MAX;
constexpr uint64_t kAggNoSlot = UINT64_MAX;

// The rows of the lanes with `in` set, folded over the wave (every lane calls this; every lane gets the result).
// base: the id of lane 0's row -- ids ascend with the lanes, so the smallest id is the lowest lane's.
__device__ __forceinline__ AggPart agg_wave_fold(bool in, unsigned long long mask, int64_t v, uint64_t base) {
    long long mn = in ? (long long)v : INT64_MAX, mx = in ? (long long)v : INT64_MIN;
    unsigned long long sum = in ? (unsigned long long)v : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        sum += __shfl_xor(sum, o);
    }
    return AggPart{(uint64_t)__builtin_popcountll(mask), mn, mx, sum, base + (uint32_t)__builtin_ctzll(mask)};
}

__device__ __forceinline__ void agg_add_lds(AggLds& t, uint32_t s, const AggPart& p) {
    (void)__hip_atomic_fetch_add(&t.count[s], (unsigned long long)p.count, AGG_RLX, AGG_WG);
    (void)__hip_atomic_fetch_min(&t.mn[s], (long long)p.mn, AGG_RLX, AGG_WG);
    (void)__hip_atomic_fetch_max(&t.mx[s], (long long)p.mx, AGG_RLX, AGG_WG);
    (void)__hip_atomic_fetch_add(&t.sum[s], (unsigned long long)p.sum, AGG_RLX, AGG_WG);
    (void)__hip_atomic_fetch_min(&t.first[s], (unsigned long long)p.first, AGG_RLX, AGG_WG);
}

__device__ __forceinline__ void agg_add_global(const AggTable& g, uint64_t s, const AggPart& p) {
    (void)__hip_atomic_fetch_add((unsigned long long*)&g.count[s], (unsigned long long)p.count, AGG_RLX, AGG_DEV);
    (void)__hip_atomic_fetch_min((long long*)&g.min_value[s], (long long)p.mn, AGG_RLX, AGG_DEV);
    (void)__hip_atomic_fetch_max((long long*)&g.max_value[s], (long long)p.mx, AGG_RLX, AGG_DEV);
    (void)__hip_atomic_fetch_add((unsigned long long*)&g.sum_value[s], (unsigned long long)p.sum, AGG_RLX, AGG_DEV);
    (void)__hip_atomic_fetch_min((unsigned long long*)&g.first_id[s], (unsigned long long)p.first, AGG_RLX, AGG_DEV);
}

// The LDS slot of `key`, claimed if it is new; kAggNoLdsSlot: neither the key nor an empty slot within the probe bound.
__device__ __forceinline__ uint32_t agg_lds_slot(AggLds& t, int64_t key) {
    if (key == kAggEmptyKey) return kAggLdsSlots;
    uint32_t s = agg_lds_home(key, kAggLdsSlots);
    for (uint32_t i = 0; i < kAggLdsProbe; ++i) {
        long long cur = __hip_atomic_load(&t.key[s], AGG_RLX, AGG_WG);
        if (cur == kAggEmptyKey && __hip_atomic_compare_exchange_strong(&t.key[s], &cur, (long long)key, AGG_RLX, AGG_RLX, AGG_WG)) return s;
        if (cur == key) return s;   // cur: what the slot held, also after a lost claim
        s = (s + 1u) & (kAggLdsSlots - 1u);
    }
    return kAggNoLdsSlot;
}

// The global slot of `key`, claimed if it is new.  kAggNoSlot: the call has failed already (too many groups), or the
// probe ran over the whole table, which the sizing rule excludes; either way the error word says so and the result is
// dropped.  A claim beyond the cap still returns its slot: adding to it is harmless.
__device__ __forceinline__ uint64_t agg_global_slot(const AggTable& g, int64_t key) {
    if (key == kAggEmptyKey) return g.slots;
    if (__hip_atomic_load((unsigned long long*)&g.ctr->err, AGG_RLX, AGG_DEV)) return kAggNoSlot;
    uint64_t s = agg_home(key, g.slots);
    for (uint64_t i = 0; i < g.slots; ++i) {
        long long cur = __hip_atomic_load((long long*)&g.key[s], AGG_RLX, AGG_DEV);
        if (cur == kAggEmptyKey && __hip_atomic_compare_exchange_strong((long long*)&g.key[s], &cur, (long long)key, AGG_RLX, AGG_RLX, AGG_DEV)) {
            if (__hip_atomic_fetch_add((unsigned long long*)&g.ctr->claimed, 1ull, AGG_RLX, AGG_DEV) >= kAggMaxGroups)
                (void)__hip_atomic_fetch_or((unsigned long long*)&g.ctr->err, (unsigned long long)kAggErrGroups, AGG_RLX, AGG_DEV);
            return s;
        }
        if (cur == key) return s;
        s = (s + 1) & (g.slots - 1);
    }
    (void)__hip_atomic_fetch_or((unsigned long long*)&g.ctr->err, (unsigned long long)kAggErrFull, AGG_RLX, AGG_DEV);
    return kAggNoSlot;
}

// Some rows of one key into the work-group's table, or past it when the key finds no room there.
__device__ __forceinline__ void agg_insert(AggLds& t, const AggTable& g, int64_t key, const AggPart& p) {
    const uint32_t s = agg_lds_slot(t, key);
    if (s != kAggNoLdsSlot) {
        agg_add_lds(t, s, p);
        return;
    }
    const uint64_t gs = agg_global_slot(g, key);
    if (gs != kAggNoSlot) agg_add_global(g, gs, p);
}

// slots + 1 entries to the identities; direct (BY_TAG): a slot's key is its index.  The counters to zero.
__global__ __launch_bounds__(256) void agg_reset_kernel(AggTable g, bool direct) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s == 0) *g.ctr = AggCounters{0ull, 0ull, 0ull, 0ull};
    if (s > g.slots) return;
    g.key[s] = direct ? (int64_t)s : kAggEmptyKey;
    g.count[s] = 0ull;
    g.min_value[s] = INT64_MAX;
    g.max_value[s] = INT64_MIN;
    g.sum_value[s] = 0ull;
    g.first_id[s] = kAggNoId;
}

// The rows in scope that match p, aggregated by key into g; g.ctr->rows += their number.  A column pointer that is null
// reads 0 in every row: the host passes only the columns the predicate and the mode need.
template <uint32_t BY>
__global__ __launch_bounds__(kAggThreads) void agg_pass_kernel(const uint64_t* __restrict__ tags, const int64_t* __restrict__ vals,
                                                               const uint32_t* __restrict__ labels, const uint32_t* __restrict__ scope,
                                                               uint64_t count, RowPred p, int64_t width, uint64_t id_offset, AggTable g) {
    constexpr uint32_t kSlots = BY == kAggByTag ? kAggTagGroups : kAggLdsSlots + 1;
    __shared__ AggLds t;
    __shared__ uint32_t part[kAggThreads / 64];
    __shared__ unsigned long long failed;
    for (uint32_t s = threadIdx.x; s < kSlots; s += kAggThreads) {
        t.key[s] = kAggEmptyKey;
        t.count[s] = 0ull;
        t.mn[s] = INT64_MAX;
        t.mx[s] = INT64_MIN;
        t.sum[s] = 0ull;
        t.first[s] = kAggNoId;
    }
    if (threadIdx.x == 0) failed = __hip_atomic_load((unsigned long long*)&g.ctr->err, AGG_RLX, AGG_DEV);
    __syncthreads();
    if (failed) return;   // the whole work-group: too many groups already, the result is dropped
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t begin = (uint64_t)blockIdx.x * kRowPredRowsPerGroup;
    uint32_t n = 0;
    for (uint32_t i = 0; i < kRowPredRowsPerGroup; i += kAggThreads) {
        const uint64_t r0 = begin + i + wave * 64;   // the wave's 64 rows: uniform
        if (r0 >= count) break;
        const uint64_t r = r0 + lane;
        const bool ok = row_in_scope(scope, r, count);
        const uint64_t tg = ok && tags ? tags[r] : 0ull;
        const int64_t v = ok && vals ? vals[r] : 0ll;
        const uint32_t l = ok && labels ? labels[r] : 0u;
        const bool hit = ok && row_pred_matches(tg, v, l, p);
        const unsigned long long bits = __ballot(hit);
        if (!bits) continue;   // uniform, as every branch around a fold below
        n += (uint32_t)__builtin_popcountll(bits);
        const uint64_t base = id_offset + r0;
        if constexpr (BY == kAggByTag) {
            unsigned long long un = hit ? tg : 0ull;   // the bits any matching row of the wave carries
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) un |= __shfl_xor(un, o);
            while (un) {
                const uint32_t b = (uint32_t)__builtin_ctzll(un);
                un &= un - 1ull;
                const bool in = hit && ((tg >> b) & 1ull);
                const AggPart pt = agg_wave_fold(in, __ballot(in), v, base);
                if (lane == 0) agg_add_lds(t, b, pt);
            }
        } else {
            const int64_t key = hit ? agg_key(BY, l, v, width) : 0ll;
            const uint32_t lead = (uint32_t)__builtin_ctzll(bits);
            const int64_t key0 = (int64_t)__shfl((long long)key, (int)lead);
            if (__ballot(hit && key == key0) == bits) {   // one key in the wave: one set of atomics for up to 64 rows
                const AggPart pt = agg_wave_fold(hit, bits, v, base);
                if (lane == lead) agg_insert(t, g, key0, pt);
            } else if (hit) {
                agg_insert(t, g, key, AggPart{1ull, v, v, (uint64_t)v, base + lane});
            }
        }
    }
    if (lane == 0) part[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
        for (uint32_t w = 0; w < kAggThreads / 64; ++w) sum += part[w];
        if (sum) (void)__hip_atomic_fetch_add((unsigned long long*)&g.ctr->rows, (unsigned long long)sum, AGG_RLX, AGG_DEV);
    }
    // the work-group's groups into the global table: one insert per distinct key
    for (uint32_t s = threadIdx.x; s < kSlots; s += kAggThreads) {
        if (!t.count[s]) continue;
        const AggPart pt{t.count[s], t.mn[s], t.mx[s], t.sum[s], t.first[s]};
        const uint64_t gs = BY == kAggByTag ? (uint64_t)s : agg_global_slot(g, s == kAggLdsSlots ? kAggEmptyKey : (int64_t)t.key[s]);
        if (gs != kAggNoSlot) agg_add_global(g, gs, pt);
    }
}

// The occupied slots (a group has at least one row) as records, in no particular order: out[0 .. min(n_out, cap)), and
// g.ctr->n_out = their number whatever cap is.  out == null only counts.
__global__ __launch_bounds__(256) void agg_compact_kernel(AggTable g, AggGroup* __restrict__ out, uint64_t cap) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > g.slots) return;
    const uint64_t c = g.count[s];
    if (!c) return;
    const uint64_t at = __hip_atomic_fetch_add((unsigned long long*)&g.ctr->n_out, 1ull, AGG_RLX, AGG_DEV);
    if (out && at < cap) out[at] = AggGroup{g.key[s], c, g.min_value[s], g.max_value[s], (int64_t)g.sum_value[s], g.first_id[s]};
}

// ------------------------------------------------------------------ launchers
void launch_agg_reset(const AggTable& g, bool direct, hipStream_t s) {
    agg_reset_kernel<<<(uint32_t)((g.slots + 1 + 255) / 256), 256, 0, s>>>(g, direct);
}

void launch_agg_pass(uint32_t by, const uint64_t* d_tags, const int64_t* d_vals, const uint32_t* d_labels, const uint32_t* d_scope,
                     uint64_t count, const RowPred& p, int64_t width, uint64_t id_offset, const AggTable& g, hipStream_t s) {
    if (!count) return;
    const uint32_t groups = agg_groups(count);
    if (by == kAggByLabel)
        agg_pass_kernel<kAggByLabel><<<groups, kAggThreads, 0, s>>>(d_tags, d_vals, d_labels, d_scope, count, p, width, id_offset, g);
    else if (by == kAggByValue)
        agg_pass_kernel<kAggByValue><<<groups, kAggThreads, 0, s>>>(d_tags, d_vals, d_labels, d_scope, count, p, width, id_offset, g);
    else
        agg_pass_kernel<kAggByTag><<<groups, kAggThreads, 0, s>>>(d_tags, d_vals, d_labels, d_scope, count, p, width, id_offset, g);
}

void launch_agg_compact(const AggTable& g, AggGroup* d_out, uint64_t cap, hipStream_t s) {
    agg_compact_kernel<<<(uint32_t)((g.slots + 1 + 255) / 256), 256, 0, s>>>(g, d_out, cap);
}

}  // namespace vrod
