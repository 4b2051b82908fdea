// snapshot_plan.h -- the host side of vrod_index_save / vrod_index_load (vrod_index.hip): the file format of an index
// snapshot (DESIGN.md "Snapshots"), its parsing and validation, the chunk arithmetic of the row stream and the section
// checksum on the host.  Plain C++ (no HIP), like search_plan.h: vrod_snapshot_info and vrod_snapshot_verify need
// nothing else, and tests/test_snapshot_abi.py drives them on a machine without a device.
//
// Version 1, little-endian.  One 4096-byte header block, then the sections, each starting on a 4096-byte boundary and
// zero-padded to the next one:
//   0    "VRODSNAP"
//   8    u32 version, dim, dtype, metric
//   24   u64 count, live_count, id_offset, file_bytes
//   56   u32 max_xn2_bits (the handle's largest squared row norm ever held, float bits), u32 n_sections
//   64   n_sections x { u32 kind, u32 0, u64 offset, u64 payload bytes, u64 checksum }, ascending offsets
//   4088 u64 checksum of bytes [0, 4088) (first_word 0)
// Everything not named is zero.  Rows are dense [count][dim] elements of the storage type: the row pitch of the handle
// that wrote them is not in the file.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>

namespace vrod {

constexpr uint32_t kSnapVersion = 1;
constexpr uint64_t kSnapBlock = 4096;          // header size and section alignment
constexpr uint64_t kSnapHeaderSumAt = 4088;    // the header's own checksum: its last 8 bytes
constexpr uint32_t kSnapTableAt = 64, kSnapEntryBytes = 32;
constexpr uint32_t kSnapMaxSections = 16;
constexpr char kSnapMagic[9] = "VRODSNAP";

enum SnapKind : uint32_t {
    SNAP_ROWS = 1,      // [count][dim] bf16 or f32, dense
    SNAP_NORMS = 2,     // [count] f32: the fast squared norms
    SNAP_DELETED = 3,   // ceil(count / 32) words, bit set = row deleted
    SNAP_FILTER = 4,    // ceil(count / 32) words, bit set = row allowed; present while a filter is set
    SNAP_LABELS = 5,    // [count] u32; present once labels were set
    SNAP_TAGS = 6,      // [count] u64; present once tags were set
    SNAP_VALUES = 7,    // [count] i64; present once values were set
    SNAP_KEYS = 8,      // [count] u64; present once keys were set (the key table is not saved: a load rebuilds it).
                        // Builds older than the kind answer VROD_ERR_UNSUPPORTED to a file that has it.
    SNAP_KIND_END = 9
};

// a save or load moves the rows in chunks of this many dense bytes (a multiple of 32 rows, at least 32) through two
// pinned host buffers; VROD_DEBUG_SNAPSHOT_CHUNK_ROWS overrides the row count
constexpr uint64_t kSnapChunkBytes = 32ull << 20;
constexpr uint64_t kSnapChunkBytesMax = 256ull << 20;   // ... whatever the override says
// sections up to this size are also verified on the host before a load touches the device: it costs nothing, and a
// bad small file fails the same way with and without a device.  Larger ones are verified by the device as they arrive.
constexpr uint64_t kSnapHostVerifyBytes = 1ull << 20;

enum SnapStatus { SNAP_OK = 0, SNAP_CORRUPT = 1, SNAP_UNSUPPORTED = 2 };

struct SnapSection {
    uint32_t kind = 0;
    uint64_t offset = 0, bytes = 0, checksum = 0;
};

struct SnapHeader {
    uint32_t version = kSnapVersion, dim = 0, dtype = 0, metric = 0;
    uint64_t count = 0, live_count = 0, id_offset = 0, file_bytes = 0;
    uint32_t max_xn2_bits = 0, n_sections = 0;
    SnapSection sections[kSnapMaxSections];
    const SnapSection* find(uint32_t kind) const {
        for (uint32_t i = 0; i < n_sections; ++i)
            if (sections[i].kind == kind) return &sections[i];
        return nullptr;
    }
};

inline uint64_t snap_round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
inline uint64_t snap_elem_bytes(uint32_t dtype) { return dtype == 1 ? 2 : 4; }

// payload bytes a section of `kind` must have in a snapshot of this shape
inline uint64_t snap_section_bytes(uint32_t kind, uint64_t count, uint32_t dim, uint32_t dtype) {
    switch (kind) {
        case SNAP_ROWS: return count * dim * snap_elem_bytes(dtype);
        case SNAP_NORMS: return count * 4;
        case SNAP_DELETED: case SNAP_FILTER: return (count + 31) / 32 * 4;
        case SNAP_LABELS: return count * 4;
        case SNAP_TAGS: case SNAP_VALUES: case SNAP_KEYS: return count * 8;
        default: return 0;
    }
}

// ---- the section checksum: sum over the payload's u32 words w_i (little-endian, the last one zero-filled) of
// mix(w_i + (first_word + i + 1) * golden), mod 2^64.  A sum: any chunking or order gives the same 64 bits.
inline uint64_t snap_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t kSnapGolden = 0x9E3779B97F4A7C15ull;
inline uint64_t snap_word_term(uint32_t w, uint64_t i) { return snap_mix((uint64_t)w + (i + 1) * kSnapGolden); }

inline uint64_t snap_checksum(const void* bytes, uint64_t n_bytes, uint64_t first_word) {
    const unsigned char* p = (const unsigned char*)bytes;
    uint64_t sum = 0;
    const uint64_t full = n_bytes / 4;
    for (uint64_t i = 0; i < full; ++i) {
        uint32_t w;
        memcpy(&w, p + i * 4, 4);
        sum += snap_word_term(w, first_word + i);
    }
    if (n_bytes % 4) {
        uint32_t w = 0;
        memcpy(&w, p + full * 4, (size_t)(n_bytes % 4));
        sum += snap_word_term(w, first_word + full);
    }
    return sum;
}

// ---- header block
inline void snap_put32(unsigned char* b, uint64_t at, uint32_t v) { memcpy(b + at, &v, 4); }
inline void snap_put64(unsigned char* b, uint64_t at, uint64_t v) { memcpy(b + at, &v, 8); }
inline uint32_t snap_get32(const unsigned char* b, uint64_t at) { uint32_t v; memcpy(&v, b + at, 4); return v; }
inline uint64_t snap_get64(const unsigned char* b, uint64_t at) { uint64_t v; memcpy(&v, b + at, 8); return v; }

// block: kSnapBlock bytes
inline void snap_encode_header(const SnapHeader& h, unsigned char* block) {
    memset(block, 0, kSnapBlock);
    memcpy(block, kSnapMagic, 8);
    snap_put32(block, 8, h.version);
    snap_put32(block, 12, h.dim);
    snap_put32(block, 16, h.dtype);
    snap_put32(block, 20, h.metric);
    snap_put64(block, 24, h.count);
    snap_put64(block, 32, h.live_count);
    snap_put64(block, 40, h.id_offset);
    snap_put64(block, 48, h.file_bytes);
    snap_put32(block, 56, h.max_xn2_bits);
    snap_put32(block, 60, h.n_sections);
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        const uint64_t at = kSnapTableAt + (uint64_t)i * kSnapEntryBytes;
        snap_put32(block, at, h.sections[i].kind);
        snap_put64(block, at + 8, h.sections[i].offset);
        snap_put64(block, at + 16, h.sections[i].bytes);
        snap_put64(block, at + 24, h.sections[i].checksum);
    }
    snap_put64(block, kSnapHeaderSumAt, snap_checksum(block, kSnapHeaderSumAt, 0));
}

// Lays the sections of `h` (kinds and bytes set, in order) out behind the header; sets offsets and file_bytes.
inline void snap_layout(SnapHeader& h) {
    uint64_t at = kSnapBlock;
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        h.sections[i].offset = at;
        at += snap_round_up(h.sections[i].bytes, kSnapBlock);
    }
    h.file_bytes = at;
}

// Parses and validates a header block of `have` bytes read from a file of `file_len` bytes.  why: a short text.
// The order is part of the contract: not a snapshot at all (CORRUPT) < a version this build does not read
// (UNSUPPORTED) < a damaged header (CORRUPT) < section kinds this build does not know (UNSUPPORTED) < sizes that
// disagree with each other or with the file (CORRUPT).
inline SnapStatus snap_parse_header(const unsigned char* block, uint64_t have, uint64_t file_len, SnapHeader& h, const char** why) {
    if (have < 8 || memcmp(block, kSnapMagic, 8) != 0) { *why = "not a vrod snapshot (magic)"; return SNAP_CORRUPT; }
    if (have < 12) { *why = "the header is cut short"; return SNAP_CORRUPT; }
    h.version = snap_get32(block, 8);
    if (h.version != kSnapVersion) { *why = "snapshot version not supported"; return SNAP_UNSUPPORTED; }
    if (have < kSnapBlock) { *why = "the header is cut short"; return SNAP_CORRUPT; }
    if (snap_get64(block, kSnapHeaderSumAt) != snap_checksum(block, kSnapHeaderSumAt, 0)) { *why = "header checksum mismatch"; return SNAP_CORRUPT; }
    h.dim = snap_get32(block, 12);
    h.dtype = snap_get32(block, 16);
    h.metric = snap_get32(block, 20);
    h.count = snap_get64(block, 24);
    h.live_count = snap_get64(block, 32);
    h.id_offset = snap_get64(block, 40);
    h.file_bytes = snap_get64(block, 48);
    h.max_xn2_bits = snap_get32(block, 56);
    h.n_sections = snap_get32(block, 60);
    if (h.n_sections > kSnapMaxSections) { *why = "too many sections"; return SNAP_CORRUPT; }
    bool unknown = false;
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        const uint64_t at = kSnapTableAt + (uint64_t)i * kSnapEntryBytes;
        h.sections[i].kind = snap_get32(block, at);
        h.sections[i].offset = snap_get64(block, at + 8);
        h.sections[i].bytes = snap_get64(block, at + 16);
        h.sections[i].checksum = snap_get64(block, at + 24);
        if (h.sections[i].kind == 0 || h.sections[i].kind >= SNAP_KIND_END) unknown = true;
    }
    if (unknown) { *why = "a section kind this version does not know"; return SNAP_UNSUPPORTED; }
    if (h.dim == 0 || h.dim > 32768u || h.dtype > 1 || h.metric > 2) { *why = "bad dim, dtype or metric"; return SNAP_CORRUPT; }
    if (h.count > 0xFFFFFF00ull || h.live_count > h.count) { *why = "bad row counts"; return SNAP_CORRUPT; }
    if (h.file_bytes != file_len) { *why = "the file's length is not the header's (truncated?)"; return SNAP_CORRUPT; }
    uint64_t at = kSnapBlock;
    uint32_t seen = 0;
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        const SnapSection& s = h.sections[i];
        if (seen & (1u << s.kind)) { *why = "a section appears twice"; return SNAP_CORRUPT; }
        seen |= 1u << s.kind;
        if (s.offset != at || s.bytes != snap_section_bytes(s.kind, h.count, h.dim, h.dtype)) {
            *why = "a section's offset or size disagrees with the header";
            return SNAP_CORRUPT;
        }
        at += snap_round_up(s.bytes, kSnapBlock);
    }
    if (at != h.file_bytes) { *why = "the sections do not add up to the file's length"; return SNAP_CORRUPT; }
    const uint32_t need = (1u << SNAP_ROWS) | (1u << SNAP_NORMS) | (1u << SNAP_DELETED);
    if ((seen & need) != need) { *why = "rows, norms or deleted-row bits are missing"; return SNAP_CORRUPT; }
    return SNAP_OK;
}

// ---- chunk arithmetic of the row stream: rows per chunk, a multiple of 32 and at least 32, so that every chunk starts
// on a word of the bitmaps and -- bf16 rows of odd dim -- on a whole u32 word of the dense payload.
// override_rows: VROD_DEBUG_SNAPSHOT_CHUNK_ROWS (0: none).
inline uint64_t snap_chunk_rows(uint32_t dim, uint32_t dtype, uint64_t override_rows) {
    const uint64_t rb = (uint64_t)dim * snap_elem_bytes(dtype);
    uint64_t rows = override_rows ? override_rows : kSnapChunkBytes / rb;
    rows = std::min(rows, kSnapChunkBytesMax / rb);
    return std::max<uint64_t>(32, rows / 32 * 32);
}
// popcount of the bits of a bitmap that name rows below `count`
inline uint64_t snap_count_bits(const uint32_t* bits, uint64_t count) {
    uint64_t n = 0;
    for (uint64_t w = 0; w < (count + 31) / 32; ++w) {
        uint32_t v = bits[w];
        if ((w + 1) * 32 > count) v &= (1u << (count - w * 32)) - 1u;
        n += (uint64_t)__builtin_popcount(v);
    }
    return n;
}

}  // namespace vrod
