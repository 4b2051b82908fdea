// ingest_plan.h -- the host decisions of the ingest (vrod_index_add, _update, _upsert, their _device forms and
// _get_rows_device; vrod_index.hip, kernels_ingest.hip): where the rows of a call come from, is a device layout valid,
// which loads may the kernel use on it, how a call is cut into chunks, how many rows share a work-group, and which shard
// of a multi-device handle gets which rows.  Plain C++ with no HIP header: tests/test_ingest_plan.py compiles it as host
// code.
#pragma once
#include <stdint.h>
#include <string.h>

namespace vrod {

// vrod_src_dtype
enum : int { SRC_F32 = 0, SRC_BF16 = 1, SRC_F16 = 2 };
inline bool ingest_dtype_known(int t) { return t == SRC_F32 || t == SRC_BF16 || t == SRC_F16; }
inline uint32_t ingest_elem_bytes(int t) { return t == SRC_F32 ? 4u : 2u; }

// What is wrong with a source (or destination) of n rows of dim elements of `dtype`, row i at element i * row_stride of
// the address `addr`: nothing, or the first of these that applies.
enum : int { INGEST_OK = 0, INGEST_BAD_DTYPE = 1, INGEST_BAD_STRIDE = 2, INGEST_OVERFLOW = 3, INGEST_MISALIGNED = 4 };
inline int ingest_check_layout(uint64_t addr, int dtype, uint64_t row_stride, uint32_t dim, uint64_t n) {
    if (!ingest_dtype_known(dtype)) return INGEST_BAD_DTYPE;
    if (row_stride < dim) return INGEST_BAD_STRIDE;   // (there is no "0 means dim")
    const uint64_t es = ingest_elem_bytes(dtype);
    // n * row_stride elements, then bytes, then the address of the last one: none may wrap 64 bits
    if (n && row_stride > UINT64_MAX / n) return INGEST_OVERFLOW;
    const uint64_t elems = n * row_stride;
    if (elems > UINT64_MAX / es) return INGEST_OVERFLOW;
    if (elems * es > UINT64_MAX - addr) return INGEST_OVERFLOW;
    if (addr % es) return INGEST_MISALIGNED;
    return INGEST_OK;
}

// Bytes per load the kernel may use: 16 where EVERY row starts on a 16-B boundary (the base does and the pitch in bytes
// is a multiple of 16), else one element.  A row's last dim % (16 / element) elements are always read one by one, so no
// load reaches into the padding behind a row or past the last row.
inline uint32_t ingest_load_bytes(uint64_t addr, int dtype, uint64_t row_stride) {
    const uint64_t es = ingest_elem_bytes(dtype);
    return (addr % 16 == 0 && (row_stride * es) % 16 == 0) ? 16u : (uint32_t)es;
}

// Where the rows of an add, update or upsert come from: fp32 rows in host memory, the synthetic stream, or typed rows in
// device memory.  Every flow above the kernels takes one of these and narrows it with the two operations below; the
// staging step of a chunk (vrod_index.hip ingest_prepare) is the only place that asks for the kind.
struct RowSource {
    enum Kind : int { HOST = 0, SYNTH = 1, DEVICE = 2 };
    Kind kind = HOST;
    const void* p = nullptr;            // HOST, DEVICE: source row 0; row i at element i * stride
    int dtype = SRC_F32;                // DEVICE: the element type (HOST: fp32)
    uint64_t stride = 0;                // HOST: dim
    int device = 0;                     // DEVICE: where p lives
    uint64_t seed = 0, first_row = 0;   // SYNTH: the stream, and the row of it that is source row 0
    // a HOST-memory list of the source rows a pass takes, in the order of the pass (null: row i of the pass is source
    // row i) -- how an update's rows reach their shards and an upsert's rows split into held and new
    const uint64_t* pick = nullptr;
};
inline RowSource rows_on_host(const float* rows, uint32_t dim) {
    RowSource s;
    s.p = rows; s.stride = dim;
    return s;
}
inline RowSource rows_synthetic(uint64_t seed, uint64_t first_row) {
    RowSource s;
    s.kind = RowSource::SYNTH; s.seed = seed; s.first_row = first_row;
    return s;
}
inline RowSource rows_on_device(const void* d_rows, int dtype, uint64_t stride) {   // (the caller finds out the device)
    RowSource s;
    s.kind = RowSource::DEVICE; s.p = d_rows; s.dtype = dtype; s.stride = stride;
    return s;
}
// the source from row `first` of the pass on
inline RowSource rows_from(const RowSource& s, uint64_t first) {
    RowSource t = s;
    if (t.pick) t.pick += first;
    else if (t.kind == RowSource::SYNTH) t.first_row += first;
    else t.p = (const char*)s.p + first * s.stride * ingest_elem_bytes(s.dtype);
    return t;
}
// the source restricted to list[0], list[1], ... of its rows (s itself is not picked)
inline RowSource rows_picked(const RowSource& s, const uint64_t* list) {
    RowSource t = s;
    t.pick = list;
    return t;
}
// rows of the run of consecutive source rows that starts at entry i of a list of m
inline uint64_t pick_run(const uint64_t* pick, uint64_t m, uint64_t i) {
    uint64_t e = i + 1;
    while (e < m && pick[e] == pick[e - 1] + 1) ++e;
    return e - i;
}
// Rows [0, m) of a picked HOST source, dense at out ([m][dim]): what the staging upload of the chunk sends.  A run of
// consecutive rows is one copy where the rows lie densely (stride == dim, as an ABI caller's do).
inline void rows_gather(const RowSource& s, uint32_t dim, uint64_t m, float* out) {
    for (uint64_t i = 0; i < m;) {
        const uint64_t run = s.stride == dim ? pick_run(s.pick, m, i) : 1;
        memcpy(out + i * dim, (const float*)s.p + s.pick[i] * s.stride, run * dim * sizeof(float));
        i += run;
    }
}

// Rows per staged chunk of an add or update of n rows: 256 MiB of raw fp32 rows at most, 65536 rows at most, 1024 at
// least.
constexpr uint64_t kIngestStageRows = 1u << 16;
inline uint64_t ingest_chunk_rows(uint64_t n, uint32_t dim) {
    uint64_t c = (256ull << 20) / (dim * 4ull);
    if (c > kIngestStageRows) c = kIngestStageRows;
    if (c < 1024) c = 1024;
    return n < c ? n : c;
}
// chunk `i` of the call: its first row and its rows (0 once the call is used up)
inline uint64_t ingest_chunk_first(uint64_t n, uint32_t dim, uint64_t i) { return i * ingest_chunk_rows(n, dim); }
inline uint64_t ingest_chunk_count(uint64_t n, uint32_t dim, uint64_t i) {
    const uint64_t c = ingest_chunk_rows(n, dim), first = i * c;
    if (!c || first >= n) return 0;
    return n - first < c ? n - first : c;
}

// A normalising work-group stages its rows in LDS as fp32, each at a pitch of dim rounded up to 4 floats (16-B reads
// feed the norm chain).  Four rows, one per wave, while they fit 64 KiB together; beyond that one row per work-group
// (VROD_MAX_DIM = 32768: 128 KiB of the CU's 160).
inline uint32_t ingest_lds_pitch(uint32_t dim) { return (dim + 3u) & ~3u; }
inline uint32_t ingest_rows_per_group(uint32_t dim) { return (uint64_t)ingest_lds_pitch(dim) * 16u <= 65536u ? 4u : 1u; }
inline uint64_t ingest_lds_bytes(uint32_t dim) { return (uint64_t)ingest_rows_per_group(dim) * ingest_lds_pitch(dim) * 4u; }

// The dealing of a multi-device handle: global row r lives on shard (r / B) % G at local row (r / (B*G)) * B + r % B,
// B = kDealBlock.  A range of rows is handed out in pieces that end at block boundaries.
constexpr uint64_t kDealBlock = 65536;
inline uint64_t deal_shard(uint64_t r, uint64_t G) { return (r / kDealBlock) % G; }
inline uint64_t deal_local_row(uint64_t r, uint64_t G) { return (r / (kDealBlock * G)) * kDealBlock + r % kDealBlock; }
// rows of the piece that starts at r and ends before `end`
inline uint64_t deal_piece_rows(uint64_t r, uint64_t end) {
    const uint64_t to_boundary = (r / kDealBlock + 1) * kDealBlock - r;
    return end - r < to_boundary ? end - r : to_boundary;
}

}  // namespace vrod
