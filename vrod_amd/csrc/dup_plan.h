// dup_plan.h -- the host decisions of duplicate-row detection (vrod_index_find_duplicates, _find_duplicates_device,
// _delete_duplicates; vrod_index.hip): the row hash, the table's size and home slot, how a (dim, element size) is read and
// how many lanes share a row (DESIGN.md "Duplicate rows").  Plain host-and-device arithmetic, no HIP runtime call
// (keys_plan.h, rowpred_plan.h): kernels_dup.hip computes what these functions define, tests/test_dup_plan.py compiles
// this header as host C++.
//
// Two live rows are duplicates when the dim stored elements of their prepared rows have the same bits.  The hash only
// decides which rows are compared; the comparison is of the rows themselves.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VROD_DUP_HD __host__ __device__
#else
#define VROD_DUP_HD
#endif

namespace vrod {

// Rows one work-group owns in the hash pass and in the class pass, restated by tests/test_gpu_duplicates.py.  With L
// lanes to a row (DupPlan::lanes) the group's 256 threads take 256 / L rows at a time, L times over.
constexpr uint32_t kDupRowsPerGroup = 256;
constexpr uint32_t kDupThreads = 256;
static_assert(kDupRowsPerGroup == kDupThreads && kDupThreads % 64 == 0, "a lane a row at one lane per row; whole waves");

// ---- the table: open addressing, linear probing, one word per slot = the row that claimed it
constexpr uint64_t kDupMinSlots = 1024;
constexpr uint32_t kDupEmpty = 0xFFFFFFFFu;    // an unclaimed slot, and the start of every slot's minimum
constexpr uint32_t kDupErrFull = 1u;           // a walk ran over every slot without an end: VROD_ERR_INTERNAL
constexpr uint32_t kDupErrSlot = 2u;           // a slot word that is neither empty nor a row below the count: likewise
// The smallest power of two that is at least 4 x live and at least kDupMinSlots: at most a quarter of the slots are
// ever claimed, so every walk meets an empty slot.
inline uint64_t dup_table_slots(uint64_t live) {
    uint64_t s = kDupMinSlots;
    while (s < 4 * live) s *= 2;
    return s;
}

// ---- the hash of a row: finish(sum over the row's 32-bit words w_i of term(w_i, i)), the last word of a bf16 row of odd
// dim zero-filled.  A sum, so any split of the words over lanes gives the same 64 bits; the two per-index keys make it
// depend on position.  One 32 x 32 -> 64 multiply a word keeps the pass bound by its loads.
constexpr uint32_t kDupKeyA = 0x9E3779B9u, kDupKeyB = 0x85EBCA6Bu;
VROD_DUP_HD inline uint64_t dup_word_term(uint32_t w, uint32_t i) {
    const uint32_t a = (i + 1u) * kDupKeyA, b = ((i + 1u) * kDupKeyB) | 1u;
    return (uint64_t)(uint32_t)(w + a) * (uint64_t)b;
}
// the snapshot checksum's mixer (snapshot_plan.h snap_mix)
VROD_DUP_HD inline uint64_t dup_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// within: VROD_DUP_WITHIN_LABEL, the class key is (label, row bits).  narrow: VROD_DUP_NARROW_HASH, 8 bits are kept.
VROD_DUP_HD inline uint64_t dup_finish(uint64_t sum, uint32_t label, bool within, bool narrow) {
    uint64_t h = dup_mix(sum + 0x9E3779B97F4A7C15ull);
    if (within) h = dup_mix(h ^ ((uint64_t)label + 1) * 0xD6E8FEB86659FD93ull);
    return narrow ? h & 0xFFull : h;
}
// mixed once more: the 256 values of a narrow hash spread over the table as the wide ones do
VROD_DUP_HD inline uint64_t dup_home(uint64_t hash, uint64_t slots) { return dup_mix(hash + 0x9E3779B97F4A7C15ull) & (slots - 1); }

// ---- how a row is read.  Rows start at row * ld and ld * esize is a multiple of 16 (of 128 on every handle), so neither
// path meets a word that straddles two rows.
enum DupRead : uint32_t {
    DUP_READ_UNITS = 0,   // dim * esize % 16 == 0: 16-byte loads, per_row of them
    DUP_READ_WORDS = 1    // otherwise: 32-bit loads, per_row = ceil(dim * esize / 4) of them, the last under tail_mask
};
struct DupPlan {
    uint32_t read;        // DupRead
    uint32_t per_row;     // loads per row: units or words
    uint32_t words;       // 32-bit words of a row's dim elements: what the hash sums over
    uint32_t tail_mask;   // the bits of the last word that belong to the row: 0xFFFF for a bf16 row of odd dim
    uint32_t lanes;       // lanes that share a row: the smallest power of two >= per_row, at most 64
};
inline DupPlan dup_plan(uint32_t dim, uint32_t esize) {
    DupPlan p{};
    const uint64_t bytes = (uint64_t)dim * esize;
    p.words = (uint32_t)((bytes + 3) / 4);
    p.tail_mask = bytes % 4 ? 0xFFFFu : 0xFFFFFFFFu;
    p.read = bytes % 16 == 0 ? DUP_READ_UNITS : DUP_READ_WORDS;
    p.per_row = p.read == DUP_READ_UNITS ? (uint32_t)(bytes / 16) : p.words;
    p.lanes = 1;
    while (p.lanes < 64 && p.lanes < p.per_row) p.lanes *= 2;
    return p;
}
// ld must keep every row's first byte on a 16-byte boundary (and so on a word)
inline bool dup_pitch_ok(uint32_t dim, uint32_t esize, uint32_t ld) { return ld >= dim && (uint64_t)ld * esize % 16 == 0; }
inline uint32_t dup_groups(uint64_t count) { return (uint32_t)((count + kDupRowsPerGroup - 1) / kDupRowsPerGroup); }

// the hash on the host: what kernels_dup.hip's hash pass writes for a row of dim elements at `row`
inline uint64_t dup_row_hash(const void* row, uint32_t dim, uint32_t esize, uint32_t label, bool within, bool narrow) {
    const DupPlan p = dup_plan(dim, esize);
    const uint64_t bytes = (uint64_t)dim * esize;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < p.words; ++i) {
        uint32_t w = 0;
        const uint64_t left = bytes - (uint64_t)i * 4;
        memcpy(&w, (const unsigned char*)row + (uint64_t)i * 4, left < 4 ? (size_t)left : 4);
        sum += dup_word_term(w, i);
    }
    return dup_finish(sum, label, within, narrow);
}

}  // namespace vrod
