// w4_steal.h -- how the 4-wave scan (kernels_mfma_w4.hip) cuts the tail of a strip into claimable chunks.  Plain
// arithmetic, no HIP headers: tests/test_w4_steal_partition.py compiles it as host C++ and checks the partition.
//
// A strip [b, e) keeps [b, e - tail) as its static share; the tail [e - tail, e) is cut into cpt = tail / kStealChunk
// chunks of kStealChunk tiles, the remainder (tail % kStealChunk) folded into the last chunk.  Every chunk is therefore
// at least 2 tiles long: the claim protocol of the kernel relies on it (a range read at a tile boundary is never the
// range wave 0 claims behind in the same advance -- see the comment at the claim in kernels_mfma_w4.hip).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define VROD_HD __host__ __device__
#else
#define VROD_HD
#endif

#ifndef VROD_W4_STEAL_CHUNK
#define VROD_W4_STEAL_CHUNK 2
#endif
#ifndef VROD_W4_STEAL_DIV
#define VROD_W4_STEAL_DIV 16
#endif

namespace vrod {

constexpr uint32_t kStealChunk = VROD_W4_STEAL_CHUNK;     // tiles per claimable chunk (the last one: up to 2x - 1)
static_assert(kStealChunk >= 2u, "a claimed range of one tile races with the claim behind it (w4_steal.h)");
static_assert(VROD_W4_STEAL_DIV >= 1, "VROD_W4_STEAL_DIV: the tail is 1/DIV of a strip");

// tiles of a strip that are handed out dynamically: 1/DIV of the strip, at most one 32-bit word of claim bits per
// (query block, strip), none on short strips (first stages, shards of small corpora) or when not one chunk fits
VROD_HD inline uint32_t w4_tail_tiles(uint32_t strip_tiles) {
    if (strip_tiles < 48u) return 0u;
    uint32_t t = strip_tiles / (uint32_t)VROD_W4_STEAL_DIV;
    if (t > 32u * kStealChunk) t = 32u * kStealChunk;
    return t < kStealChunk ? 0u : t;
}
// chunks of the tail of a strip of `strip_tiles` tiles (<= 32)
VROD_HD inline uint32_t w4_tail_chunks(uint32_t strip_tiles) { return w4_tail_tiles(strip_tiles) / kStealChunk; }
// tiles [cb, ce) of chunk j < w4_tail_chunks(e - b) of the strip [b, e)
VROD_HD inline void w4_chunk_range(uint32_t b, uint32_t e, uint32_t j, uint32_t& cb, uint32_t& ce) {
    const uint32_t tail = w4_tail_tiles(e - b);
    cb = e - tail + j * kStealChunk;
    ce = j + 1u == tail / kStealChunk ? e : cb + kStealChunk;
}

}  // namespace vrod
