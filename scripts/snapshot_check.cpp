// snapshot_check.cpp -- a stand-alone, host-only reader of index snapshots: snapshot_plan.h (header parsing, validation,
// the section checksum) and nothing else of the library.  No HIP, no device.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o snapshot_check scripts/snapshot_check.cpp
//   ./snapshot_check FILE...      one line per file: "FILE: ok ..." or "FILE: corrupt|unsupported|io: why"
//
// It exists so that the parser can be run under AddressSanitizer and UBSan over sound and damaged files (tests/
// test_snapshot_abi.py writes both kinds); the exit status is 0 when every file got a verdict, whatever the verdict.
#include <stdio.h>

#include <vector>

#include "../vrod_amd/csrc/snapshot_plan.h"

using namespace vrod;

static void check(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { printf("%s: io: cannot open\n", path); return; }
    std::vector<unsigned char> raw;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + n);
    fclose(f);
    SnapHeader h;
    const char* why = "";
    const SnapStatus st = snap_parse_header(raw.data(), std::min<uint64_t>(raw.size(), kSnapBlock), raw.size(), h, &why);
    if (st != SNAP_OK) { printf("%s: %s: %s\n", path, st == SNAP_UNSUPPORTED ? "unsupported" : "corrupt", why); return; }
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        const SnapSection& s = h.sections[i];
        // in two pieces, to exercise first_word: a sum, so the pieces add up
        const uint64_t half = s.bytes / 8 * 4;
        const uint64_t sum = snap_checksum(raw.data() + s.offset, half, 0) + snap_checksum(raw.data() + s.offset + half, s.bytes - half, half / 4);
        if (sum != s.checksum) { printf("%s: corrupt: checksum mismatch in section %u\n", path, s.kind); return; }
    }
    const SnapSection* del = h.find(SNAP_DELETED);
    std::vector<uint32_t> bits((size_t)(del->bytes / 4));
    if (del->bytes) memcpy(bits.data(), raw.data() + del->offset, (size_t)del->bytes);
    if (h.count - snap_count_bits(bits.data(), h.count) != h.live_count) { printf("%s: corrupt: live count\n", path); return; }
    unsigned char again[kSnapBlock];
    snap_encode_header(h, again);
    printf("%s: ok version %u dim %u dtype %u metric %u count %llu live %llu sections %u chunk_rows %llu reencoded %s\n", path, h.version, h.dim,
           h.dtype, h.metric, (unsigned long long)h.count, (unsigned long long)h.live_count, h.n_sections,
           (unsigned long long)snap_chunk_rows(h.dim, h.dtype, 0), memcmp(again, raw.data(), kSnapBlock) == 0 ? "same" : "DIFFERENT");
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) check(argv[i]);
    return 0;
}
