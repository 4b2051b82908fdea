// kernels_dup.hip -- the device side of duplicate-row detection (vrod_index_find_duplicates, _find_duplicates_device,
// _delete_duplicates; gfx950): the classes of live rows whose dim stored elements have the same bits, found in one
// streaming read of the corpus plus a hash table in device memory.  The host decisions are in dup_plan.h.
//
// The reference stores whatever it is given and has no notion of a copy (src/database/mod.rs: insert appends); here a
// corpus with exact copies pays for them at search time (DESIGN.md "Duplicate rows"), so the handle can list them.
//
// Three passes.  L = DupPlan::lanes consecutive lanes share a row in the first two -- one lane for a row of one 16-byte
// unit, the whole wave for a row of 64 units or more -- and a work-group owns kDupRowsPerGroup consecutive rows:
//   hash    THE HOT PATH: every live row is read once, 16 bytes a lane where dim * esize % 16 == 0 and a word a lane
//           otherwise, each lane sums dup_word_term over its share, L lanes add up by xor shuffles, 8 bytes per row are
//           written.  No reuse, so no LDS: pure streaming.
//   class   a row walks the table from dup_home(hash).  An empty slot is claimed by a 32-bit atomicCAS with the row's own
//           index; an occupied one names its owner, whose hash is compared and then -- the L lanes together -- the row
//           itself.  Equal: that slot is the row's class.  Different: a miss, the walk goes on.  The class's smallest
//           row is an atomicMin into slot_min.
//   output  out_first[r] = id_offset + slot_min[row_slot[r]], the class sizes (an atomicAdd per row on the class's first
//           row), the counts, and for a delete the bitmap of the rows that are not their class's first.
// NO THREAD EVER WAITS FOR ANOTHER.  A slot word goes from empty to a row index once and never changes again; the row
// index is all a reader needs, because rows and hashes do not change during the call.  Rows with equal bits walk the
// same slots past the same owners, so a class has exactly one slot, whichever of its rows claimed it.  Every walk is
// bounded by the slot count: one that runs out raises kDupErrFull and ends (VROD_ERR_INTERNAL), as the key table's do.
// Every shuffle and ballot is executed by the whole wave: the loops are wave-uniform and a row's state is predicated.
#include "dup_plan.h"
#include "dup_read.h"
#include "vrod_common.h"
#include "vrod_kernels.h"

namespace vrod {

// The row a thread works on in step `it` of its group: 256 / L rows a step, lanes [g * L, (g + 1) * L) of the group on one.
__device__ __forceinline__ uint64_t dup_row_of(uint32_t it, uint32_t lanes_log2) {
    return (uint64_t)blockIdx.x * kDupRowsPerGroup + ((uint64_t)it << (8u - lanes_log2)) + (threadIdx.x >> lanes_log2);
}
static_assert(kDupThreads == 256, "dup_row_of: 256 >> lanes_log2 rows a step");
// ... and the row of the first lane of the thread's wave: the same for the whole wave
__device__ __forceinline__ uint64_t dup_row_of_wave(uint32_t it, uint32_t lanes_log2) {
    return (uint64_t)blockIdx.x * kDupRowsPerGroup + ((uint64_t)it << (8u - lanes_log2)) + ((threadIdx.x & ~63u) >> lanes_log2);
}

// hash[r] for every live row r < count.  Deleted rows are neither read nor written.
template <typename P>
__global__ __launch_bounds__(kDupThreads) void dup_hash_kernel(const unsigned char* __restrict__ corpus, uint64_t row_bytes, uint64_t count,
                                                               const uint32_t* __restrict__ del, const uint32_t* __restrict__ labels,
                                                               uint32_t per_row, uint32_t tail_mask, uint32_t lanes_log2, bool within, bool narrow,
                                                               uint64_t* __restrict__ hash) {
    const uint32_t L = 1u << lanes_log2, sub = threadIdx.x & (L - 1u);
    for (uint32_t it = 0; it < L; ++it) {
        const uint64_t r = dup_row_of(it, lanes_log2);
        if (dup_row_of_wave(it, lanes_log2) >= count) break;   // the wave's first row: uniform, and later steps lie higher
        const bool live = r < count && !dup_row_dead(del, r);
        const unsigned char* row = corpus + r * row_bytes;
        uint64_t s = 0;
        for (uint32_t j0 = 0; j0 < per_row; j0 += L) {   // uniform trip count; a lane without a load adds nothing
            const uint32_t j = j0 + sub;
            if (live && j < per_row) s += P::terms(P::cut(P::load(row, j), j + 1u == per_row, tail_mask), j);
        }
        for (uint32_t o = L >> 1; o > 0; o >>= 1) s += (uint64_t)__shfl_xor((unsigned long long)s, (int)o);
        if (live && sub == 0) hash[r] = dup_finish(s, within && labels ? labels[r] : 0u, within, narrow);
    }
}

// The table after the launch: slot_row[s] = the row that claimed slot s, slot_min[s] = the smallest row of its class;
// row_slot[r] = the slot of live row r.  slot_row and slot_min are all-ones before the launch, *ctr is zero.
template <typename P>
__global__ __launch_bounds__(kDupThreads) void dup_class_kernel(const unsigned char* __restrict__ corpus, uint64_t row_bytes, uint64_t count,
                                                                const uint32_t* __restrict__ del, const uint32_t* __restrict__ labels,
                                                                uint32_t per_row, uint32_t tail_mask, uint32_t lanes_log2, bool within,
                                                                const uint64_t* __restrict__ hash, uint32_t* __restrict__ slot_row,
                                                                uint32_t* __restrict__ slot_min, uint64_t slots, uint32_t* __restrict__ row_slot,
                                                                DupCounters* __restrict__ ctr) {
    const uint32_t L = 1u << lanes_log2, lane = threadIdx.x & 63u, sub = lane & (L - 1u), lead = lane & ~(L - 1u);
    const unsigned long long sub_mask = L == 64u ? ~0ull : ((1ull << L) - 1ull) << lead;
    const uint64_t mask = slots - 1;
    unsigned long long misses = 0;
    uint32_t longest = 0, err = 0;
    for (uint32_t it = 0; it < L; ++it) {
        const uint64_t r = dup_row_of(it, lanes_log2);
        if (dup_row_of_wave(it, lanes_log2) >= count) break;   // the wave's first row: uniform, and later steps lie higher
        const bool live = r < count && !dup_row_dead(del, r);
        const unsigned char* row = corpus + r * row_bytes;
        const uint64_t h = live ? hash[r] : 0ull;
        const uint32_t lab = live && within && labels ? labels[r] : 0u;
        uint64_t s = dup_home(h, slots);
        bool walking = live;   // the same for the L lanes of a row
        uint32_t found = kDupEmpty, steps = 0;
        for (uint64_t p = 0; p < slots; ++p) {   // bounded by the table; leaves when no row of the wave walks any more
            if (!__ballot(walking)) break;
            uint32_t cur = kDupEmpty;
            if (walking && sub == 0) {   // the row's first lane reads the slot and claims it when it is empty
                cur = slot_row[s];
                if (cur == kDupEmpty) {
                    cur = atomicCAS(&slot_row[s], kDupEmpty, (uint32_t)r);
                    if (cur == kDupEmpty) cur = (uint32_t)r;   // claimed: the row is its own slot's owner
                }
            }
            cur = (uint32_t)__shfl((int)cur, (int)lead);
            bool same = false;   // the owner may be this row's class: its hash (and label) agree
            if (walking) {
                ++steps;
                if (cur == (uint32_t)r) { found = (uint32_t)s; walking = false; }
                else if (cur >= count) { err |= kDupErrSlot; walking = false; }
                else same = hash[cur] == h && (!within || !labels || labels[cur] == lab);
            }
            if (__ballot(same)) {   // the full comparison, a row's lanes together
                const unsigned char* other = corpus + (uint64_t)(same ? cur : 0u) * row_bytes;
                bool diff = false;
                for (uint32_t j0 = 0; j0 < per_row; j0 += L) {
                    const uint32_t j = j0 + sub;
                    if (same && j < per_row) {
                        const bool last = j + 1u == per_row;
                        diff |= P::differs(P::cut(P::load(row, j), last, tail_mask), P::cut(P::load(other, j), last, tail_mask));
                    }
                }
                const bool differs = (__ballot(diff) & sub_mask) != 0ull;
                if (same) {
                    if (differs) misses += sub == 0;
                    else { found = (uint32_t)s; walking = false; }
                }
            }
            if (walking) s = (s + 1) & mask;
        }
        if (walking) err |= kDupErrFull;
        if (live && sub == 0 && found != kDupEmpty) {
            atomicMin(&slot_min[found], (uint32_t)r);
            row_slot[r] = found;
        }
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

// One thread per row, whole 64-row waves.  first = slot_min[row_slot[r]] for a live row: out_first[r] (may be null) =
// id_offset + first, all-ones for a deleted row; class_size[first] (zero before the launch) counts the class, and the
// last to add sees its size; hits (may be null; the words of the rows below count rounded up to 64): bit r set = row r is
// live and not its class's first.  Writes nothing when the class pass raised an error.
__global__ __launch_bounds__(256) void dup_output_kernel(uint64_t count, const uint32_t* __restrict__ del, const uint32_t* __restrict__ row_slot,
                                                         const uint32_t* __restrict__ slot_min, uint64_t id_offset, uint64_t* __restrict__ out_first,
                                                         uint32_t* __restrict__ class_size, uint32_t* __restrict__ hits, DupCounters* __restrict__ ctr) {
    if (ctr->err) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, end = (count + 63) / 64 * 64;
    unsigned long long classes = 0;
    uint32_t largest = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < end; r += stride) {
        const bool live = r < count && !dup_row_dead(del, r);
        uint32_t first = kDupEmpty;
        if (live) {
            first = slot_min[row_slot[r]];
            largest = max(largest, atomicAdd(&class_size[first], 1u) + 1u);
            classes += first == (uint32_t)r;
        }
        if (out_first && r < count) out_first[r] = live ? id_offset + first : UINT64_MAX;
        const unsigned long long bits = __ballot(live && first != (uint32_t)r);
        if (hits && (lane & 31u) == 0u) hits[r >> 5] = (uint32_t)(lane ? bits >> 32 : bits);
    }
    for (int o = 32; o > 0; o >>= 1) {
        classes += __shfl_xor(classes, o);
        largest = max(largest, (uint32_t)__shfl_xor((int)largest, o));
    }
    if (lane == 0) {
        if (classes) atomicAdd(&ctr->classes, classes);
        if (largest) atomicMax(&ctr->largest_class, largest);
    }
}

// ------------------------------------------------------------------ launchers
static uint32_t dup_log2(uint32_t lanes) { uint32_t l = 0; while ((1u << l) < lanes) ++l; return l; }

void launch_dup_hash(const void* d_corpus, uint32_t dim, uint32_t ld, uint32_t esize, uint64_t count, const uint32_t* d_del, const uint32_t* d_labels,
                     bool within, bool narrow, uint64_t* d_hash, hipStream_t s) {
    if (!count) return;
    const DupPlan p = dup_plan(dim, esize);
    const unsigned char* c = (const unsigned char*)d_corpus;
    const uint64_t rb = (uint64_t)ld * esize;
    if (p.read == DUP_READ_UNITS)
        dup_hash_kernel<DupUnits><<<dup_groups(count), kDupThreads, 0, s>>>(c, rb, count, d_del, d_labels, p.per_row, p.tail_mask, dup_log2(p.lanes), within, narrow, d_hash);
    else
        dup_hash_kernel<DupWords><<<dup_groups(count), kDupThreads, 0, s>>>(c, rb, count, d_del, d_labels, p.per_row, p.tail_mask, dup_log2(p.lanes), within, narrow, d_hash);
}

void launch_dup_class(const void* d_corpus, uint32_t dim, uint32_t ld, uint32_t esize, uint64_t count, const uint32_t* d_del, const uint32_t* d_labels,
                      bool within, const uint64_t* d_hash, const DupTable& T, DupCounters* d_ctr, hipStream_t s) {
    if (!count) return;
    const DupPlan p = dup_plan(dim, esize);
    const unsigned char* c = (const unsigned char*)d_corpus;
    const uint64_t rb = (uint64_t)ld * esize;
    if (p.read == DUP_READ_UNITS)
        dup_class_kernel<DupUnits><<<dup_groups(count), kDupThreads, 0, s>>>(c, rb, count, d_del, d_labels, p.per_row, p.tail_mask, dup_log2(p.lanes), within, d_hash,
                                                                           T.slot_row, T.slot_min, T.slots, T.row_slot, d_ctr);
    else
        dup_class_kernel<DupWords><<<dup_groups(count), kDupThreads, 0, s>>>(c, rb, count, d_del, d_labels, p.per_row, p.tail_mask, dup_log2(p.lanes), within, d_hash,
                                                                           T.slot_row, T.slot_min, T.slots, T.row_slot, d_ctr);
}

void launch_dup_output(uint64_t count, const uint32_t* d_del, const DupTable& T, uint64_t id_offset, uint64_t* d_out_first, uint32_t* d_class_size,
                       uint32_t* d_hits, DupCounters* d_ctr, hipStream_t s) {
    if (!count) return;
    const unsigned grid = (unsigned)std::min<uint64_t>(2048, (count + 255) / 256);
    dup_output_kernel<<<grid, 256, 0, s>>>(count, d_del, T.row_slot, T.slot_min, id_offset, d_out_first, d_class_size, d_hits, d_ctr);
}

}  // namespace vrod
