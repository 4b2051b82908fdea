// kernels_rowfind.hip -- the device side of row lookup (vrod_index_find_rows, _add_unique and their _device forms;
// gfx950): the join between a batch of prepared inputs and the corpus.  The host decisions are in rowfind_plan.h, the
// flow in vrod_index.hip (DESIGN.md "Row lookup").
//
// The reference stores whatever it is given (src/database/mod.rs: insert appends) and cannot say whether a vector is
// in it already; here the handle answers from the rows themselves.
//
// A batch's staged rows are a small corpus: kernels_dup.hip hashes them and builds their classes in a table of their
// own (slot_row[s] = the staged row that owns slot s, slot_min[s] = the smallest staged row of its class).  Then:
//   probe    THE HOT PATH: one lane per corpus row streams the row's 8-byte hash and its tombstone bit -- a dead row is
//            skipped by its bit, whatever the hash array holds for it -- and walks the BATCH's table from dup_home(hash).
//            An empty slot ends the walk: no input has these bits.  A slot whose owner's hash agrees is a candidate, and
//            the candidates of a wave are compared one after the other BY THE WHOLE WAVE: the ballot names the lanes that
//            hold one, each pair (corpus row, staged row) is broadcast and read by 64 lanes under DupPlan's read rule
//            (16-byte units, or words with the last one masked).  Equal: atomicMin(found[slot], row) and the walk ends,
//            since equal rows share one slot.  Different: a miss, the walk goes on.  8 bytes per corpus row, plus two
//            rows per candidate.
//   resolve  one thread per input: the class's found row (the corpus's first, else the side corpus's) and its first
//            input of the batch, 16 bytes per input for the host.
//   keep     the batch's new inputs, listed by the host: their hashes go behind the corpus's (the rows add_unique has
//            appended), and for find_rows their staged rows go to the call's side corpus.
// No thread waits for another; every walk is bounded by the slot count (kDupErrFull); every ballot and shuffle is
// executed by the whole wave: the loops are wave-uniform and a row's state is predicated.
#include "dup_plan.h"
#include "dup_read.h"
#include "rowfind_plan.h"
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

// found[s] (all-ones before) = the smallest live row r < count whose dim stored elements equal those of staged row
// slot_row[s].  count < 2^32 - 256 (a shard's limit), so a row fits the slot word and the shuffles.
template <typename P>
__global__ __launch_bounds__(256) void rowfind_probe_kernel(const unsigned char* __restrict__ corpus, uint64_t row_bytes, uint64_t count,
                                                            const uint32_t* __restrict__ del, const uint64_t* __restrict__ hash,
                                                            const unsigned char* __restrict__ stage, uint32_t m,
                                                            const uint64_t* __restrict__ stage_hash, const uint32_t* __restrict__ slot_row,
                                                            uint64_t slots, uint32_t per_row, uint32_t tail_mask, uint32_t* __restrict__ found,
                                                            DupCounters* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t mask = slots - 1, stride = (uint64_t)gridDim.x * blockDim.x, end = (count + 63) / 64 * 64;
    unsigned long long misses = 0;
    uint32_t longest = 0, err = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < end; r += stride) {   // whole waves: uniform
        const bool live = r < count && !dup_row_dead(del, r);
        const uint64_t h = live ? hash[r] : 0ull;
        uint64_t s = dup_home(h, slots);
        bool walking = live;
        uint32_t steps = 0;
        for (uint64_t p = 0; p < slots; ++p) {   // bounded by the table; leaves when no row of the wave walks any more
            if (!__ballot(walking)) break;
            uint32_t cur = kDupEmpty;
            bool same = false;   // the slot's owner may have this row's bits: its hash agrees
            if (walking) {
                ++steps;
                cur = slot_row[s];
                if (cur == kDupEmpty) walking = false;                             // no input of the batch has these bits
                else if (cur >= m) { err |= kDupErrSlot; walking = false; }
                else same = stage_hash[cur] == h;
            }
            unsigned long long todo = __ballot(same);
            while (todo) {   // one candidate pair at a time, the whole wave reading it
                const int l = __ffsll(todo) - 1;
                todo &= todo - 1;
                const uint32_t rr = (uint32_t)__shfl((int)(uint32_t)r, l), cc = (uint32_t)__shfl((int)cur, l);
                const unsigned char* a = corpus + (uint64_t)rr * row_bytes;
                const unsigned char* b = stage + (uint64_t)cc * row_bytes;
                bool diff = false;
                for (uint32_t j = lane; j < per_row; j += 64u) {
                    const bool last = j + 1u == per_row;
                    diff |= P::differs(P::cut(P::load(a, j), last, tail_mask), P::cut(P::load(b, j), last, tail_mask));
                }
                const bool differs = __ballot(diff) != 0ull;
                if ((int)lane == l) {
                    if (differs) ++misses;
                    else { atomicMin(&found[s], (uint32_t)r); walking = false; }   // equal rows share one slot: the walk is over
                }
            }
            if (walking) s = (s + 1) & mask;
        }
        if (walking) err |= kDupErrFull;
        longest = max(longest, steps);
    }
    for (int o = 32; o > 0; o >>= 1) {
        misses += __shfl_xor(misses, o);
        longest = max(longest, (uint32_t)__shfl_xor((int)longest, o));
        err |= (uint32_t)__shfl_xor((int)err, o);
    }
    if (lane == 0) {
        if (misses) atomicAdd(&ctr->compare_misses, misses);
        if (longest) atomicMax(&ctr->max_probe, longest);
        if (err) atomicOr(&ctr->err, err);
    }
}

// ans[i] for input i < m of the batch (rowfind_plan.h RowfindAnswer).  found_side may be null: no side corpus.  Writes
// nothing when a pass raised an error.
__global__ __launch_bounds__(256) void rowfind_resolve_kernel(uint32_t m, const uint32_t* __restrict__ row_slot, const uint32_t* __restrict__ slot_min,
                                                              const uint32_t* __restrict__ found, const uint32_t* __restrict__ found_side,
                                                              uint64_t count0, RowfindAnswer* __restrict__ ans, const DupCounters* __restrict__ ctr) {
    if (ctr->err) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = row_slot[i], f = found[s], g = found_side ? found_side[s] : kDupEmpty;
    RowfindAnswer a;
    a.row = f != kDupEmpty ? (uint64_t)f : g != kDupEmpty ? count0 + g : kRowfindNone;
    a.first = slot_min[s];
    ans[i] = a;
}

// New input j < k of the batch is staged row news[j]: dst_hash[j] = its hash, and (dst_rows not null) row j of dst_rows =
// its staged row, row_bytes (a multiple of 16) each, 16 bytes a lane.
__global__ __launch_bounds__(256) void rowfind_keep_kernel(const unsigned char* __restrict__ stage, uint64_t row_bytes,
                                                           const uint64_t* __restrict__ stage_hash, const uint32_t* __restrict__ news, uint32_t k,
                                                           unsigned char* __restrict__ dst_rows, uint64_t* __restrict__ dst_hash) {
    const uint32_t units = (uint32_t)(row_bytes / 16);
    for (uint32_t j = blockIdx.x; j < k; j += gridDim.x) {
        const uint32_t src = news[j];
        if (threadIdx.x == 0) dst_hash[j] = stage_hash[src];
        if (!dst_rows) continue;
        const u32x4_t* from = reinterpret_cast<const u32x4_t*>(stage + (uint64_t)src * row_bytes);
        u32x4_t* to = reinterpret_cast<u32x4_t*>(dst_rows + (uint64_t)j * row_bytes);
        for (uint32_t u = threadIdx.x; u < units; u += blockDim.x) to[u] = from[u];
    }
}

// ------------------------------------------------------------------ launchers
void launch_rowfind_probe(const void* d_corpus, uint32_t dim, uint32_t ld, uint32_t esize, uint64_t count, const uint32_t* d_del, const uint64_t* d_hash,
                          const void* d_stage, uint32_t m, const uint64_t* d_stage_hash, const DupTable& T, uint32_t* d_found, DupCounters* d_ctr,
                          hipStream_t s) {
    if (!count || !m) return;
    const DupPlan p = dup_plan(dim, esize);
    const uint64_t rb = (uint64_t)ld * esize;
    const unsigned grid = (unsigned)std::min<uint64_t>(2048, (count + 255) / 256);
    if (p.read == DUP_READ_UNITS)
        rowfind_probe_kernel<DupUnits><<<grid, 256, 0, s>>>((const unsigned char*)d_corpus, rb, count, d_del, d_hash, (const unsigned char*)d_stage, m,
                                                            d_stage_hash, T.slot_row, T.slots, p.per_row, p.tail_mask, d_found, d_ctr);
    else
        rowfind_probe_kernel<DupWords><<<grid, 256, 0, s>>>((const unsigned char*)d_corpus, rb, count, d_del, d_hash, (const unsigned char*)d_stage, m,
                                                            d_stage_hash, T.slot_row, T.slots, p.per_row, p.tail_mask, d_found, d_ctr);
}

void launch_rowfind_resolve(uint32_t m, const DupTable& T, const uint32_t* d_found, const uint32_t* d_found_side, uint64_t count0, RowfindAnswer* d_ans,
                            const DupCounters* d_ctr, hipStream_t s) {
    if (!m) return;
    rowfind_resolve_kernel<<<(m + 255) / 256, 256, 0, s>>>(m, T.row_slot, T.slot_min, d_found, d_found_side, count0, d_ans, d_ctr);
}

void launch_rowfind_keep(const void* d_stage, uint32_t ld, uint32_t esize, const uint64_t* d_stage_hash, const uint32_t* d_news, uint32_t k,
                         void* d_dst_rows, uint64_t* d_dst_hash, hipStream_t s) {
    if (!k) return;
    rowfind_keep_kernel<<<std::min<uint32_t>(k, 4096u), 256, 0, s>>>((const unsigned char*)d_stage, (uint64_t)ld * esize, d_stage_hash, d_news, k,
                                                                     (unsigned char*)d_dst_rows, d_dst_hash);
}

}  // namespace vrod
