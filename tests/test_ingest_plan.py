"""The host decisions of the ingest (vrod_amd/csrc/ingest_plan.h), checked on the host: a small driver is compiled with
g++ against the real header.

  - the row source of a call (host rows, the synthetic stream, device rows): what "from row `first` on" and "these rows
    of it" make of each kind, and the gather of a picked host source into the dense chunk its upload sends;
  - layout validation: a stride below dim, n * row_stride (elements, bytes, end address) past 64 bits, a pointer that is
    not aligned to its element, an unknown element type; and which loads a pointer and pitch allow;
  - the chunk cuts of a call at n = chunk - 1, chunk, chunk + 1 (and around them), against the rule the host forms state;
  - the rows per work-group and the LDS they take, up to VROD_MAX_DIM;
  - the dealing of rows to the shards of a multi-device handle, against the ranges the host add hands out."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
MAX_DIM = int(re.search(r"#define VROD_MAX_DIM (\d+)u", open(os.path.join(ROOT, "include", "vrod.h")).read()).group(1))
U64 = 1 << 64
OK, BAD_DTYPE, BAD_STRIDE, OVERFLOW, MISALIGNED = range(5)

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "ingest_plan.h"
using namespace vrod;

int main() {
    char what;
    printf("M %llu %llu %d %d %d\n", (unsigned long long)kIngestStageRows, (unsigned long long)kDealBlock, SRC_F32, SRC_BF16, SRC_F16);
    while (scanf(" %c", &what) == 1) {
        if (what == 'L') {          // layout: addr dtype stride dim n
            unsigned long long addr, stride, n; int dt; unsigned dim;
            scanf("%llu %d %llu %u %llu", &addr, &dt, &stride, &dim, &n);
            printf("L %d %u\n", ingest_check_layout(addr, dt, stride, dim, n), ingest_dtype_known(dt) ? ingest_load_bytes(addr, dt, stride) : 0u);
        } else if (what == 'C') {   // chunks: n dim
            unsigned long long n; unsigned dim;
            scanf("%llu %u", &n, &dim);
            printf("C %llu", (unsigned long long)ingest_chunk_rows(n, dim));
            for (uint64_t i = 0;; ++i) {
                const uint64_t m = ingest_chunk_count(n, dim, i);
                if (!m) break;
                printf(" %llu:%llu", (unsigned long long)ingest_chunk_first(n, dim, i), (unsigned long long)m);
            }
            printf("\n");
        } else if (what == 'G') {   // work-group: dim
            unsigned dim;
            scanf("%u", &dim);
            printf("G %u %u %llu\n", ingest_lds_pitch(dim), ingest_rows_per_group(dim), (unsigned long long)ingest_lds_bytes(dim));
        } else if (what == 'F') {   // the source from row `first` on, per kind: first -> byte offset of p, stream row, list offset
            unsigned long long first;
            scanf("%llu", &first);
            static const float host[4] = {0};
            static const uint64_t list[4] = {0};
            const RowSource src[4] = {rows_on_host(host, 5), rows_synthetic(9, 100), rows_on_device(host, SRC_F16, 7),
                                      rows_picked(rows_on_device(host, SRC_F32, 7), list)};
            printf("F");
            for (const RowSource& s : src) {
                const RowSource t = rows_from(s, first);
                printf(" %d:%lld:%llu:%lld", (int)t.kind, (long long)((const char*)t.p - (const char*)s.p), (unsigned long long)t.first_row,
                       t.pick ? (long long)(t.pick - list) : -1ll);
            }
            printf("\n");
        } else if (what == 'P') {   // gather: dim stride m pick[m], over host rows with element j of row i = 1000 i + j
            unsigned dim, stride, m;
            scanf("%u %u %u", &dim, &stride, &m);
            std::vector<uint64_t> pick(m);
            uint64_t top = 0;
            for (uint64_t& x : pick) { unsigned long long v; scanf("%llu", &v); x = v; top = v > top ? v : top; }
            std::vector<float> rows((top + 1) * stride, -1.0f), out((size_t)m * dim, -2.0f);
            for (uint64_t i = 0; i <= top; ++i) for (unsigned j = 0; j < dim; ++j) rows[i * stride + j] = 1000.0f * i + j;
            const RowSource s = rows_picked(rows_on_host(rows.data(), stride), pick.data());
            rows_gather(s, dim, m, out.data());
            printf("P");
            for (uint64_t i = 0; i < m;) { const uint64_t run = pick_run(pick.data(), m, i); printf(" %llu", (unsigned long long)run); i += run; }
            printf(" |");
            for (float v : out) printf(" %g", v);
            printf("\n");
        } else {                    // dealing: first n G -> pieces shard:global_first:local_first:rows
            unsigned long long first, n, G;
            scanf("%llu %llu %llu", &first, &n, &G);
            printf("D");
            for (uint64_t r = first; r < first + n;) {
                const uint64_t m = deal_piece_rows(r, first + n);
                printf(" %llu:%llu:%llu:%llu", (unsigned long long)deal_shard(r, G), (unsigned long long)r,
                       (unsigned long long)deal_local_row(r, G), (unsigned long long)m);
                r += m;
            }
            printf("\n");
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("ingest_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_constants_follow_the_abi_and_the_package(run):
    import vrod_amd
    hdr = open(os.path.join(ROOT, "include", "vrod.h")).read()
    enum = re.search(r"typedef enum \{ VROD_SRC_F32 = (\d), VROD_SRC_BF16 = (\d), VROD_SRC_F16 = (\d) \} vrod_src_dtype;", hdr).groups()
    f = run("")[0].split()
    assert f == ["M", "65536", "65536", *enum]
    assert [int(x) for x in enum] == [vrod_amd.SRC_F32, vrod_amd.SRC_BF16, vrod_amd.SRC_F16] == [0, 1, 2]


def test_layout_validation(run):
    A = 0x7F0000000000   # a 16-byte aligned address
    cases = [
        # addr, dtype, stride, dim, n -> verdict, load bytes
        ((A, 0, 768, 768, 10), (OK, 16)),
        ((A, 0, 767, 768, 10), (BAD_STRIDE, 4)),             # stride < dim
        ((A, 0, 0, 768, 10), (BAD_STRIDE, 16)),              # there is no "0 means dim"
        ((A, 0, 0, 768, 0), (BAD_STRIDE, 16)),               # ... whatever n is
        ((A, 3, 768, 768, 10), (BAD_DTYPE, 0)),
        ((A, -1, 768, 768, 10), (BAD_DTYPE, 0)),
        ((A, 0, 769, 768, 10), (OK, 4)),                     # rows on 4-byte boundaries only
        ((A, 0, 772, 768, 10), (OK, 16)),
        ((A + 4, 0, 772, 768, 10), (OK, 4)),
        ((A + 2, 0, 768, 768, 10), (MISALIGNED, 4)),         # fp32 at a 2-byte address
        ((A + 2, 1, 768, 768, 10), (OK, 2)),                 # bf16 / fp16 may sit there
        ((A + 1, 2, 768, 768, 10), (MISALIGNED, 2)),
        ((A, 1, 768, 768, 10), (OK, 16)),
        ((A, 2, 769, 768, 10), (OK, 2)),                     # rows on 2-byte boundaries only
        ((A, 2, 776, 768, 10), (OK, 16)),                    # 776 * 2 bytes is a multiple of 16
        ((A, 1, 772, 768, 10), (OK, 2)),                     # 772 * 2 is not
        ((A, 0, 1, 1, 1), (OK, 4)),
        ((A, 0, U64 // 2, 768, 2), (OVERFLOW, 16)),          # n * stride = 2^64
        ((A, 0, U64 // 2 - 1, 768, 2), (OVERFLOW, 4)),       # the elements fit, their bytes do not
        ((A, 1, (U64 - A) // 2 - 8, 1, 1), (OK, 16)),        # the last byte lies below 2^64
        ((A, 1, (U64 - A) // 2, 1, 1), (OVERFLOW, 16)),      # the end address is 2^64: it wraps
        ((A, 0, U64 - 1, 768, 1), (OVERFLOW, 4)),
        ((A, 0, U64 - 1, 768, 0), (OK, 4)),                  # no rows: nothing to overflow
    ]
    out = run("".join("L %d %d %d %d %d\n" % c for c, _ in cases))[1:]
    assert len(out) == len(cases)
    for (c, want), line in zip(cases, out):
        assert tuple(int(x) for x in line.split()[1:]) == want, (c, line)


def test_row_source_from_and_picked(run):
    out = run("F 0\nF 3\n")[1:]
    # host fp32 rows of 5, the synthetic stream from row 100, fp16 device rows 7 apart, a picked device source
    assert out[0].split()[1:] == ["0:0:0:-1", "1:0:100:-1", "2:0:0:-1", "2:0:0:0"]
    assert out[1].split()[1:] == ["0:60:0:-1", "1:0:103:-1", "2:42:0:-1", "2:0:0:3"]   # a picked source moves along its list only


def test_gather_of_a_picked_host_source(run):
    cases = [(3, 3, [0]), (3, 3, [4, 5, 6]), (3, 3, [6, 5, 4]), (2, 3, [1, 2, 2, 3, 4, 9, 0, 1]), (1, 1, [7, 8, 2, 3, 4]), (5, 5, [2, 0, 1])]
    out = run("".join(f"P {d} {st} {len(p)} {' '.join(map(str, p))}\n" for d, st, p in cases))[1:]
    assert len(out) == len(cases)
    for (dim, _, pick), line in zip(cases, out):
        runs, vals = line[2:].split("|")
        want_runs, i = [], 0
        while i < len(pick):                                   # consecutive source rows travel as one copy
            e = i + 1
            while e < len(pick) and pick[e] == pick[e - 1] + 1:
                e += 1
            want_runs.append(e - i)
            i = e
        assert [int(x) for x in runs.split()] == want_runs, (pick, line)
        assert [float(x) for x in vals.split()] == [1000.0 * r + j for r in pick for j in range(dim)], (pick, line)


def chunk_rule(n, dim):
    """Rows per chunk as vrod_index_add states it: 256 MiB of raw fp32 rows at most, 65536 at most, 1024 at least."""
    return min(n, max(1024, min(65536, (256 << 20) // (dim * 4))))


def test_chunk_cuts(run):
    grid = []
    for dim in (1, 64, 768, 1024, 1025, 4096, 32768):
        c = chunk_rule(1 << 40, dim)
        for n in sorted({1, 2, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c + 5}):
            grid.append((n, dim))
    grid.append((65536 + 5, 64))
    out = run("".join(f"C {n} {d}\n" for n, d in grid))[1:]
    assert len(out) == len(grid)
    for (n, dim), line in zip(grid, out):
        f = line.split()
        c = chunk_rule(n, dim)
        assert int(f[1]) == c, (n, dim, line)
        parts = [tuple(int(x) for x in p.split(":")) for p in f[2:]]
        assert len(parts) == -(-n // c)
        at = 0
        for i, (first, m) in enumerate(parts):   # in order, no gap, only the last one ragged
            assert first == at and 0 < m <= c and (m == c or i == len(parts) - 1), (n, dim, parts)
            at += m
        assert at == n
    assert chunk_rule(1 << 40, 32768) == 2048 and chunk_rule(1 << 40, 1025) == 65472 and chunk_rule(1 << 40, 64) == 65536


def test_rows_per_work_group_and_lds(run):
    dims = [1, 3, 4, 63, 64, 65, 768, 769, 4095, 4096, 4097, 16384, MAX_DIM]
    out = run("".join(f"G {d}\n" for d in dims))[1:]
    for dim, line in zip(dims, out):
        pitch, rows, lds = (int(x) for x in line.split()[1:])
        assert pitch == -(-dim // 4) * 4 and pitch >= dim          # 16-byte LDS reads feed the norm chain
        assert rows == (4 if pitch * 16 <= 65536 else 1), dim      # a wave per row while four rows fit 64 KiB
        assert lds == rows * pitch * 4 and lds <= 160 * 1024, dim  # within the CU's LDS at every legal dim
    assert out[dims.index(4096)].split()[2] == "4" and out[dims.index(4097)].split()[2] == "1"


def host_add_ranges(first, n, G, B=65536):
    """The pieces vrod_index_add hands to the shards of a G-device handle for global rows [first, first + n): cut at
    every block boundary, block b on shard b % G at local block b // G."""
    out, r, end = [], first, first + n
    while r < end:
        b = r // B
        m = min(end, (b + 1) * B) - r
        out.append((b % G, r, (b // G) * B + r % B, m))
        r += m
    return out


def test_dealing_matches_the_host_add(run):
    B = 65536
    grid = [(0, 1, 2), (0, B, 2), (0, B + 1, 2), (B - 1, 2, 2), (B - 3, 3 * B + 7, 3), (5 * B + 11, 4 * B, 4), (123, 10 * B, 8),
            (2 * B, B, 1), (7 * B - 1, 1, 5), (0, 0, 2)]
    out = run("".join(f"D {a} {n} {g}\n" for a, n, g in grid))[1:]
    assert len(out) == len(grid)
    for (first, n, G), line in zip(grid, out):
        got = [tuple(int(x) for x in p.split(":")) for p in line.split()[1:]]
        assert got == host_add_ranges(first, n, G), (first, n, G)
        # every shard's local rows are handed out densely and in order
        nxt = {}
        for g, _, local, m in host_add_ranges(0, first + n, G):
            assert nxt.get(g, 0) == local
            nxt[g] = local + m
