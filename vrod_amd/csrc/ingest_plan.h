// ingest_plan.h -- the host decisions of the device-resident ingest (vrod_index_add_device, _update_device,
// _upsert_device, _get_rows_device; vrod_index.hip, kernels_ingest.hip): is a source layout valid, which loads may the
// kernel use on it, how a call is cut into chunks, how many rows share a work-group, and which shard of a multi-device
// handle gets which rows.  Plain C++ with no HIP header: tests/test_ingest_plan.py compiles it as host code.
#pragma once
#include <stdint.h>

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

// Rows per staged chunk of an add or update of n rows: 256 MiB of raw fp32 rows at most, 65536 rows at most, 1024 at
// least (the host forms' chunks: vrod_index.hip stage_chunk_rows is this function).
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
