// kernels_near.hip -- near-duplicate classes: the connected components of the threshold graph (vrod_index_find_near_duplicates,
// _delete_near_duplicates; gfx950).
//
// The edges come from range scans whose queries are stored rows (vrod_index.hip near_run); what is here joins them:
//   near_init_kernel     parent[r] = r, class_size[r] = 0: every row a component of its own;
//   near_union_kernel    one thread per entry of a batch's hit pool: the two rows of the entry are united in a lock-free
//                        union-find over parent[] -- find with path halving, then the larger root linked under the smaller
//                        by compare-and-swap -- so a root is always the smallest row of its component, whatever order the
//                        entries arrive in;
//   near_flatten_kernel  out_first[r] = find(r) + id_offset (all-ones for a row that is not eligible), the components'
//                        sizes, the counts, and for a delete the bitmap of the rows that are not their component's root.
//
// Invariant: parent[x] <= x, equal exactly for a root, and parent[x] is an ancestor of x that stays one.  A word of
// parent[] changes in two ways only: a root hi gets a smaller root lo (the CAS), and a row that is not a root gets a
// smaller ancestor (atomicMin).  Both lower it: PARENTS ONLY EVER DECREASE, a row that stopped being a root never is one
// again, and a find walk, which goes to a strictly smaller row at every step, ends within `count` steps.  A failed CAS
// means the larger root stopped being one, so its next find ends strictly lower: the sum of the two roots falls with
// every retry, and a union retries at most 2 * count times.  Both bounds are counted; a walk that runs out raises the
// error word (near_plan.h) and ends.  No thread waits for another.
//
// Every read of parent[] inside a launch that also writes it is a device-scope atomic load: a CU's L1 is not refreshed by
// other CUs' atomics, and a walk that kept reading a stale word could use up its bound without being wrong.
#include "kernels_range.h"
#include "near_plan.h"
#include "vrod_common.h"

namespace vrod {

__device__ __forceinline__ uint32_t near_parent(const uint32_t* parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool near_bit(const uint32_t* __restrict__ bits, uint64_t r) { return (bits[r >> 5] >> (r & 31)) & 1u; }

// The root of x's component at some moment of the walk; rows on the way are pointed at their grandparents.
__device__ inline uint32_t near_find(uint32_t* parent, uint32_t x, uint32_t count, uint32_t& err) {
    for (uint32_t steps = 0; steps <= count; ++steps) {
        const uint32_t p = near_parent(parent, x);
        if (p == x) return x;
        const uint32_t g = near_parent(parent, p);
        if (g == p) { x = p; continue; }   // p was a root a moment ago: the next step confirms it or goes on
        atomicMin(parent + x, g);
        x = g;
    }
    err |= kNearErrWalk;
    return x;
}

__device__ inline void near_unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t count, uint32_t& err) {
    const uint64_t bound = 2ull * count;
    for (uint64_t tries = 0; tries <= bound; ++tries) {
        a = near_find(parent, a, count, err);
        b = near_find(parent, b, count, err);
        if (err || a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
        a = hi;   // no root any more: its find ends below hi now
        b = lo;
    }
    err |= kNearErrRetry;
}

__global__ __launch_bounds__(256) void near_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ class_size, uint64_t count) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < count; r += stride) {
        parent[r] = (uint32_t)r;
        class_size[r] = 0u;
    }
}

__global__ __launch_bounds__(256) void near_union_kernel(const RangeHit* __restrict__ hits, uint64_t stored, const uint32_t* __restrict__ batch_rows,
                                                         uint32_t batch_n, uint64_t id_offset, uint32_t count, uint32_t* parent,
                                                         NearCounters* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long pairs = 0;
    uint32_t err = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < stored; i += stride) {
        const RangeHit h = hits[i];
        const uint64_t q = h.key >> 32, b = h.id - id_offset;
        if (q >= batch_n || b >= count) { err |= kNearErrRow; continue; }
        const uint32_t a = batch_rows[q];
        if (a >= count) { err |= kNearErrRow; continue; }
        if (a == (uint32_t)b) continue;   // the row's hit on itself
        ++pairs;
        near_unite(parent, a, (uint32_t)b, count, err);
    }
    for (int o = 32; o > 0; o >>= 1) {
        pairs += __shfl_xor(pairs, o);
        err |= (uint32_t)__shfl_xor((int)err, o);
    }
    if (lane == 0) {
        if (pairs) atomicAdd(&ctr->hits, pairs);
        if (err) atomicOr(&ctr->err, err);
    }
}

// One thread per row, whole 64-row waves (the pattern of dup_output_kernel).  class_size[root] counts the component and
// the last to add sees its size; hits: the words of the rows below count rounded up to 64.
__global__ __launch_bounds__(256) void near_flatten_kernel(uint64_t count, const uint32_t* __restrict__ mask, uint32_t* parent, uint64_t id_offset,
                                                           uint64_t* __restrict__ out_first, uint32_t* __restrict__ class_size,
                                                           uint32_t* __restrict__ hits, NearCounters* ctr) {
    if (__hip_atomic_load(&ctr->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // (one load per wave: its lanes agree)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, end = (count + 63) / 64 * 64;
    unsigned long long classes = 0, rows = 0;
    uint32_t largest = 0, err = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < end; r += stride) {
        const bool elig = r < count && !(mask && near_bit(mask, r));
        uint32_t root = 0xFFFFFFFFu;
        if (elig) {
            root = near_find(parent, (uint32_t)r, (uint32_t)count, err);
            largest = max(largest, atomicAdd(&class_size[root], 1u) + 1u);
            classes += root == (uint32_t)r;
            ++rows;
        }
        if (out_first && r < count) out_first[r] = elig ? id_offset + root : UINT64_MAX;
        const unsigned long long bits = __ballot(elig && root != (uint32_t)r);
        if (hits && (lane & 31u) == 0u) hits[r >> 5] = (uint32_t)(lane ? bits >> 32 : bits);
    }
    for (int o = 32; o > 0; o >>= 1) {
        classes += __shfl_xor(classes, o);
        rows += __shfl_xor(rows, o);
        largest = max(largest, (uint32_t)__shfl_xor((int)largest, o));
        err |= (uint32_t)__shfl_xor((int)err, o);
    }
    if (lane == 0) {
        if (classes) atomicAdd(&ctr->classes, classes);
        if (rows) atomicAdd(&ctr->rows, rows);
        if (largest) atomicMax(&ctr->largest_class, largest);
        if (err) atomicOr(&ctr->err, err);
    }
}

// ------------------------------------------------------------------ launchers
static unsigned near_grid(uint64_t n) { return (unsigned)std::min<uint64_t>(2048, (n + 255) / 256); }

void launch_near_init(uint32_t* d_parent, uint32_t* d_class_size, uint64_t count, hipStream_t s) {
    if (!count) return;
    near_init_kernel<<<near_grid(count), 256, 0, s>>>(d_parent, d_class_size, count);
}

void launch_near_union(const RangeHit* d_hits, uint64_t stored, const uint32_t* d_batch_rows, uint32_t batch_n, uint64_t id_offset, uint64_t count,
                       uint32_t* d_parent, NearCounters* d_ctr, hipStream_t s) {
    if (!stored) return;
    near_union_kernel<<<near_grid(stored), 256, 0, s>>>(d_hits, stored, d_batch_rows, batch_n, id_offset, (uint32_t)count, d_parent, d_ctr);
}

void launch_near_flatten(uint64_t count, const uint32_t* d_mask, uint32_t* d_parent, uint64_t id_offset, uint64_t* d_out_first, uint32_t* d_class_size,
                         uint32_t* d_hits, NearCounters* d_ctr, hipStream_t s) {
    if (!count) return;
    near_flatten_kernel<<<near_grid(count), 256, 0, s>>>(count, d_mask, d_parent, id_offset, d_out_first, d_class_size, d_hits, d_ctr);
}

}  // namespace vrod
