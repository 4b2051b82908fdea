// compact_plan.h -- the host side of vrod_index_compact (vrod_index.hip): how the live rows of a corpus with deleted
// rows move down IN PLACE, the id map a caller gets back, and the compaction of a per-row bit vector (the filter's
// allowed bits).  Plain C++ (no HIP), like search_plan.h: tests/test_compact_plan.py compiles it with g++.
//
// A live row s moves to d = s - (deleted rows below s) <= s, so one launch over the whole corpus could overwrite rows
// another work-group has not read yet.  The corpus is therefore walked in ascending chunks, one after another on one
// stream.  Chunk [r0, r1) with L live rows goes to [w0, w0 + L), w0 = live rows below r0 <= r0:
//   - w0 + L is the number of live rows below r1, so it is <= r1: the destination never reaches a later chunk's
//     source, and every earlier chunk is already consumed;
//   - it may overlap the chunk's OWN source while w0 + L > r0: such a chunk is STAGED (its live rows are gathered
//     into a staging buffer, then copied to the destination);
//   - once w0 + L <= r0 the chunk is DIRECT: one gather kernel, one read and one write per live byte.
// Rows below the first deleted row do not move: the first chunk starts at that row's 32-row word.
// Chunk boundaries are multiples of 32, so a chunk covers whole words of the deleted-row bitmap.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace vrod {

// rows per staged chunk of a compaction at most (a multiple of 32): the staging buffer holds one such chunk
constexpr uint64_t kCompactChunkRows = 1u << 16;

struct CompactChunk {
    uint64_t r0 = 0, r1 = 0;   // source rows [r0, r1), r0 % 32 == 0
    uint64_t w0 = 0, L = 0;    // its L live rows become rows [w0, w0 + L)
    bool staged = false;       // through the staging buffer (w0 + L > r0), else moved directly
};

struct CompactPlan {
    uint64_t live = 0;                  // rows that survive = the new count
    uint64_t first_moved = 0;           // rows below it stay where they are (= count when nothing is deleted)
    std::vector<CompactChunk> chunks;   // ascending, disjoint; every live row from first_moved on is in exactly one
};

inline bool bit_of(const uint32_t* bits, uint64_t i) { return (bits[i / 32] >> (i % 32)) & 1u; }

// the bits of word w that name rows below `count`
inline uint32_t valid_bits(uint64_t w, uint64_t count) {
    if ((w + 1) * 32 <= count) return ~0u;
    return w * 32 >= count ? 0u : (1u << (count - w * 32)) - 1u;
}

// del: ceil(count / 32) words, bit set = row deleted (bits at or above `count` are ignored).
// Words without a live row belong to no chunk.  At a gap (rows already freed below the next live word) of at least a
// quarter of chunk_rows the next chunk is direct and runs on for as long as its live rows fit the gap -- the gap only
// grows, so the direct chunks grow with it; below that a chunk takes chunk_rows rows through the staging buffer.
inline CompactPlan plan_compact(const uint32_t* del, uint64_t count, uint64_t chunk_rows = kCompactChunkRows) {
    CompactPlan p;
    chunk_rows = std::max<uint64_t>(32, chunk_rows / 32 * 32);
    const uint64_t min_direct = std::max<uint64_t>(32, chunk_rows / 4);
    const uint64_t words = (count + 31) / 32;
    auto live_in = [&](uint64_t w) { return (uint64_t)__builtin_popcount(~del[w] & valid_bits(w, count)); };
    uint64_t w = 0, live = 0;
    for (; w < words; ++w) {   // whole words without a deleted row stay
        const uint32_t v = valid_bits(w, count);
        if (del[w] & v) break;
        live += (uint64_t)__builtin_popcount(v);
    }
    p.first_moved = std::min(w * 32, count);
    while (w < words) {
        if (!live_in(w)) { ++w; continue; }
        CompactChunk c;
        c.r0 = w * 32;
        c.w0 = live;
        const uint64_t gap = c.r0 - c.w0;
        if (gap >= min_direct) {
            for (; w < words && c.L + live_in(w) <= gap; ++w) c.L += live_in(w);
        } else {
            for (const uint64_t end = std::min(words, w + chunk_rows / 32); w < end; ++w) c.L += live_in(w);
        }
        c.r1 = std::min(count, w * 32);
        c.staged = c.w0 + c.L > c.r0;
        live += c.L;
        p.chunks.push_back(c);
    }
    p.live = live;
    return p;
}

// word_base[w] = live rows below row 32 * w: with the word's own bits, every live row's destination
// (d = word_base[s / 32] + popcount(~del[s / 32] & ((1 << s % 32) - 1))).  ceil(count / 32) entries.
inline void compact_word_bases(const uint32_t* del, uint64_t count, uint32_t* word_base) {
    uint64_t live = 0;
    for (uint64_t w = 0; w * 32 < count; ++w) {
        word_base[w] = (uint32_t)live;
        live += (uint64_t)__builtin_popcount(~del[w] & valid_bits(w, count));
    }
}

// out[i] = the new id of old row i (offset applied), or UINT64_MAX for a deleted row.  `count` entries.
inline void compact_new_ids(const uint32_t* del, uint64_t count, uint64_t offset, uint64_t* out) {
    uint64_t live = 0;
    for (uint64_t i = 0; i < count; ++i) out[i] = bit_of(del, i) ? UINT64_MAX : offset + live++;
}

// The bits of the surviving rows, in their new places: out bit d = bits bit s for the d-th live row s.  `out` holds
// `out_words` words and is cleared first; bits of rows at or above `count` are ignored.  Returns the survivors.
inline uint64_t compact_bits(const uint32_t* del, const uint32_t* bits, uint64_t count, uint32_t* out, uint64_t out_words) {
    std::fill(out, out + out_words, 0u);
    uint64_t d = 0;
    for (uint64_t w = 0; w * 32 < count; ++w) {
        uint32_t keep = ~del[w] & valid_bits(w, count);
        while (keep) {
            const uint32_t b = (uint32_t)__builtin_ctz(keep);
            keep &= keep - 1u;
            if ((bits[w] >> b) & 1u) out[d / 32] |= 1u << (d % 32);
            ++d;
        }
    }
    return d;
}

// The same for a column of one word per row (labels, tags, values, keys): out[d] = col[s] for the d-th live row s, and
// the vacated tail out[survivors, count) takes `none`.  `out` holds `count` entries, apart from `col`; nothing beyond
// them is written.  Returns the survivors.
template <typename T>
inline uint64_t compact_column(const uint32_t* del, const T* col, uint64_t count, T none, T* out) {
    uint64_t d = 0;
    for (uint64_t s = 0; s < count; ++s)
        if (!bit_of(del, s)) out[d++] = col[s];
    std::fill(out + d, out + count, none);
    return d;
}

}  // namespace vrod
