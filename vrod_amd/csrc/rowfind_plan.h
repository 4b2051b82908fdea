// rowfind_plan.h -- the host decisions of row lookup (vrod_index_find_rows, _add_unique and their _device forms;
// vrod_index.hip, kernels_rowfind.hip, DESIGN.md "Row lookup"): which flag bits exist, how a call is cut into lookup
// batches, how large a batch's class table is, and how the device's answer for an input becomes its id.  Plain C++ with
// no HIP header: tests/test_rowfind_plan.py compiles it as host code.  The row hash and the table's size are dup_plan.h's
// and the chunking is ingest_plan.h's: both are called here, neither is restated.
#pragma once
#include <stdint.h>

#include "dup_plan.h"
#include "ingest_plan.h"

namespace vrod {

constexpr uint32_t kRowfindNarrowHash = 0x80000000u;   // VROD_ROWFIND_NARROW_HASH
constexpr uint32_t kRowfindSmallBatch = 0x40000000u;   // VROD_ROWFIND_SMALL_BATCH
constexpr uint64_t kRowfindSmallRows = 96;             // rows of a lookup batch under it: a wave and a half
constexpr uint64_t kRowfindNone = ~0ull;               // VROD_ID_NONE
inline bool rowfind_flags_ok(uint32_t flags) { return (flags & ~(kRowfindNarrowHash | kRowfindSmallBatch)) == 0; }

// ---- the lookup batches: the chunks of an add (ingest_chunk_rows), or 96 rows under the diagnostic flag
inline uint64_t rowfind_batch_rows(uint64_t n, uint32_t dim, bool small) {
    if (small) return n < kRowfindSmallRows ? n : kRowfindSmallRows;
    return ingest_chunk_rows(n, dim);
}
inline uint64_t rowfind_batches(uint64_t n, uint32_t dim, bool small) {
    const uint64_t b = rowfind_batch_rows(n, dim, small);
    return b ? (n + b - 1) / b : 0;
}
// batch `i` of the call: its first input and its inputs (0 once the call is used up)
inline uint64_t rowfind_batch_first(uint64_t n, uint32_t dim, bool small, uint64_t i) { return i * rowfind_batch_rows(n, dim, small); }
inline uint64_t rowfind_batch_count(uint64_t n, uint32_t dim, bool small, uint64_t i) {
    const uint64_t b = rowfind_batch_rows(n, dim, small), first = i * b;
    if (!b || first >= n) return 0;
    return n - first < b ? n - first : b;
}
// a batch's staged rows are a small corpus without deletions: its class table is the one find_duplicates would build
inline uint64_t rowfind_table_slots(uint64_t batch_rows) { return dup_table_slots(batch_rows); }

// ---- what the device says of one input of a batch (16 bytes: all that crosses to the host per input)
// row:   the smallest row equal to the input among the live rows of the corpus AS THE BATCH'S PROBE SAW IT, kRowfindNone
//        when there is none.  Rows below count0 (the count when the call began) were stored before the call; row
//        count0 + j stands for the j-th NEW input of the earlier batches of this call -- appended there by add_unique,
//        kept beside the corpus by find_rows.
// first: the smallest input of the same batch with the input's prepared bits, as an index into the batch (itself when it
//        is the first).
struct RowfindAnswer {
    uint64_t row;
    uint64_t first;
};

struct RowfindTotals {
    uint64_t found = 0, repeats = 0, fresh = 0;   // fresh: the call's new inputs so far (add_unique appends them)
};

// The resolution rule, for the m inputs [i0, i0 + m) of one batch in call order.  out_ids: the WHOLE call's array, inputs
// below i0 resolved already; new_inputs: the whole call's list of new inputs (room for n), T.fresh of them known before.
// append: add_unique, a new input takes id_offset + count0 + its place among the new inputs; else it gets kRowfindNone.
// news[0 .. return value): the batch's new inputs as indices into the batch, ascending.
inline uint64_t rowfind_resolve(const RowfindAnswer* ans, uint64_t i0, uint64_t m, uint64_t count0, uint64_t id_offset, bool append,
                                uint64_t* out_ids, uint64_t* new_inputs, uint32_t* news, RowfindTotals& T) {
    uint64_t k = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const RowfindAnswer a = ans[i];
        if (a.row != kRowfindNone && a.row < count0) {          // a live row stored before the call
            out_ids[i0 + i] = id_offset + a.row;
            T.found++;
        } else if (a.row != kRowfindNone) {                     // a new input of an earlier batch
            out_ids[i0 + i] = out_ids[new_inputs[a.row - count0]];
            T.repeats++;
        } else if (a.first != i) {                              // an earlier input of this batch
            out_ids[i0 + i] = out_ids[i0 + a.first];
            T.repeats++;
        } else {                                                // new
            out_ids[i0 + i] = append ? id_offset + count0 + T.fresh : kRowfindNone;
            new_inputs[T.fresh++] = i0 + i;
            news[k++] = (uint32_t)i;
        }
    }
    return k;
}

}  // namespace vrod
