// near_plan.h -- the host decisions of near-duplicate detection (vrod_index_find_near_duplicates, _device,
// _delete_near_duplicates; vrod_index.hip): which flags exist, how the eligible rows are cut into batches of range
// queries, how large the hit pool of a call is, and how a batch whose hits overflow it is redone (DESIGN.md
// "Near-duplicate rows").  Plain arithmetic, no HIP headers (byid_plan.h, dup_plan.h): vrod_index.hip enqueues what these
// functions decide, kernels_near.hip raises the error words defined here, tests/test_near_plan.py compiles this header as
// host C++.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "byid_plan.h"

namespace vrod {

// The flag bits of the ABI (VROD_NEAR_SMALL_POOL, include/vrod.h); anything else is refused.
constexpr uint32_t kNearSmallPool = 0x80000000u;
inline bool near_flags_ok(uint32_t flags) { return (flags & ~kNearSmallPool) == 0; }

// ---- the error word of the union-find kernels: a bounded walk that ran out, VROD_ERR_INTERNAL on the host
constexpr uint32_t kNearErrWalk = 1u;    // a find walk took more than `count` steps
constexpr uint32_t kNearErrRetry = 2u;   // a link was retried more than 2 * count times
constexpr uint32_t kNearErrRow = 4u;     // a hit names a row that is not below the count

// ---- the hit pool: entries (16 bytes each) a batch's qualifying (query, row) pairs are appended to before the union
// pass reads them.  A fixed budget -- 4 Mi entries, 64 MiB: 4096 hits per query of a full bf16 batch -- but never fewer
// entries than there are eligible rows: one query's hits are at most the eligible rows, so a one-row batch always fits
// and the halving below always ends.  small_pool (the diagnostic flag): exactly the eligible count, so that batches
// split on a corpus of a few thousand rows.
constexpr uint64_t kNearPoolBudget = 1ull << 22;
inline uint64_t near_pool_entries(uint64_t eligible, bool small_pool) {
    return small_pool ? eligible : std::max<uint64_t>(kNearPoolBudget, eligible);
}

// ---- batches: consecutive pieces of the ascending list of eligible rows.  The first cut is the graph's (byid_plan.h:
// 1024 rows over bf16 storage, 256 over fp32 -- the sizes the batched scan was measured at), the last batch partial.
struct NearBatch { uint64_t first; uint32_t rows; };   // positions [first, first + rows) of the eligible list
inline uint32_t near_batch_rows(bool bf16, uint64_t eligible) { return byid_batch_rows(bf16, eligible); }
inline uint64_t near_n_batches(uint64_t eligible, uint32_t batch) { return byid_n_batches(eligible, batch); }
inline NearBatch near_batch(uint64_t eligible, uint32_t batch, uint64_t s) {
    const ByidBatch b = byid_batch(eligible, batch, s);
    return {b.first, b.rows};
}

// A batch's exact hit total against the pool: it fits, it is redone as two halves, or -- one row, which cannot overflow
// a pool of at least the eligible count -- something is wrong.
enum NearVerdict { NEAR_FITS = 0, NEAR_SPLIT = 1, NEAR_IMPOSSIBLE = 2 };
inline NearVerdict near_verdict(const NearBatch& b, uint64_t total, uint64_t pool_entries) {
    if (total <= pool_entries) return NEAR_FITS;
    return b.rows > 1 ? NEAR_SPLIT : NEAR_IMPOSSIBLE;
}
// The two halves of a batch of at least two rows: the lower one takes the odd row; both are non-empty and together
// they are the batch.
inline void near_halves(const NearBatch& b, NearBatch* lo, NearBatch* hi) {
    const uint32_t h = b.rows - b.rows / 2;
    *lo = {b.first, h};
    *hi = {b.first + h, b.rows - h};
}

}  // namespace vrod
