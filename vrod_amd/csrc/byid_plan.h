// byid_plan.h -- the host decisions of the searches whose queries are stored rows (vrod_search_by_ids, vrod_knn_graph):
// how many results the underlying search asks for, and how vrod_knn_graph cuts its id range into batches -- the batch
// size, the number of batches, the tail batch, and which of the two in-flight workspaces each batch uses.  Plain
// arithmetic, no HIP headers (search_plan.h, group_plan.h): vrod_index.hip enqueues what these functions decide,
// tests/test_byid_plan.py compiles this header as host C++.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace vrod {

// The largest k of the ABI (VROD_MAX_K, include/vrod.h).
constexpr uint32_t kByidMaxK = 3584;

// Results per query of the underlying search: with the self drop one more than the caller's k -- the top k of S \ {self}
// is the top (k + 1) of S with self removed -- which is why k stops at kByidMaxK - 1 there.
inline uint32_t byid_search_k(uint32_t k, bool exclude_self) { return exclude_self ? k + 1 : k; }
inline bool byid_k_ok(uint32_t k, bool exclude_self) { return k >= 1 && byid_search_k(k, exclude_self) <= kByidMaxK; }

// Rows per batch of the graph: the batch sizes the batched (MFMA) scan was tuned and measured at -- 1024 queries over
// bf16 rows (the 4-wave kernel's four query blocks of 256), 256 over fp32 rows (the split pass's measured batch: its
// query planes and hit lists are three times a bf16 batch's).  A range shorter than a batch is one batch: `n` only
// caps the size, so the results never depend on it.
constexpr uint32_t kByidBatchBf16 = 1024, kByidBatchF32 = 256;
inline uint32_t byid_batch_rows(bool bf16, uint64_t n) {
    const uint32_t b = bf16 ? kByidBatchBf16 : kByidBatchF32;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(b, n));
}

inline uint64_t byid_n_batches(uint64_t n, uint32_t batch) { return (n + batch - 1) / batch; }

// Batch s of a range of n rows: rows [first, first + rows) of the range -- consecutive, in order, the last one partial --
// and the workspace it uses.  Two batches are in flight at most (s and s + 1), so alternating slots never collide.
struct ByidBatch { uint64_t first; uint32_t rows; uint32_t slot; };
inline ByidBatch byid_batch(uint64_t n, uint32_t batch, uint64_t s) {
    const uint64_t first = s * batch;
    return {first, (uint32_t)std::min<uint64_t>(batch, n - first), (uint32_t)(s & 1)};
}

}  // namespace vrod
