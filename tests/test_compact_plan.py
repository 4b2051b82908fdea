"""The host-side plan of vrod_index_compact (vrod_amd/csrc/compact_plan.h), checked on the host: a small driver is
compiled with g++ against the real header, reads tombstone patterns and prints, for each, the chunk plan, the per-word
destination bases, the new-id map, a compacted bit vector and two compacted row columns (a 4-byte one whose default is
0 and an 8-byte one whose default is every bit set).  Everything is compared with a numpy restatement:

  - every live row is read exactly once (the chunks are ascending and disjoint, the rows between them are all
    deleted); rows below the first moved row are live and stay; a staged chunk fits the staging buffer;
  - destinations are dense and order-preserving (w0 = live rows below r0, L = live rows of the chunk);
  - a chunk marked direct has w0 + L <= r0, a staged one does not;
  - no chunk's destination reaches a later chunk's source;
  - the id map, the word bases and the compacted allow bits equal numpy's;
  - a compacted column holds the survivors' words in order, then its default up to the count, and nothing beyond."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
ID_NONE = 0xFFFFFFFFFFFFFFFF

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "compact_plan.h"
using namespace vrod;

int main() {
    unsigned long long count, chunk, offset;
    while (scanf("%llu %llu %llu", &count, &chunk, &offset) == 3) {
        const size_t words = (size_t)((count + 31) / 32);
        std::vector<uint32_t> del(words + 1), bits(words + 1), out(words + 3, 0xDEADBEEFu), base(words + 1);
        for (size_t w = 0; w < words; ++w) scanf("%x", &del[w]);
        for (size_t w = 0; w < words; ++w) scanf("%x", &bits[w]);
        const CompactPlan p = chunk ? plan_compact(del.data(), count, chunk) : plan_compact(del.data(), count);
        printf("P %llu %llu %zu\n", (unsigned long long)p.live, (unsigned long long)p.first_moved, p.chunks.size());
        for (const CompactChunk& c : p.chunks)
            printf("C %llu %llu %llu %llu %d\n", (unsigned long long)c.r0, (unsigned long long)c.r1, (unsigned long long)c.w0,
                   (unsigned long long)c.L, (int)c.staged);
        compact_word_bases(del.data(), count, base.data());
        printf("W");
        for (size_t w = 0; w < words; ++w) printf(" %u", base[w]);
        printf("\n");
        std::vector<uint64_t> ids(count + 1);
        compact_new_ids(del.data(), count, offset, ids.data());
        printf("M");
        for (unsigned long long i = 0; i < count; ++i) printf(" %llu", (unsigned long long)ids[i]);
        printf("\n");
        const unsigned long long n = compact_bits(del.data(), bits.data(), count, out.data(), words + 2);
        printf("B %llu", n);
        for (size_t w = 0; w < words + 3; ++w) printf(" %x", out[w]);
        printf("\n");
        // the row columns: word r of each is a fixed function of r (COL4 / COL8 below), two canaries past the count
        std::vector<uint32_t> col4(count + 1), out4(count + 2, 0xDEADBEEFu);
        std::vector<uint64_t> col8(count + 1), out8(count + 2, 0xDEADBEEFDEADBEEFull);
        for (unsigned long long r = 0; r < count; ++r) { col4[r] = (uint32_t)r * 2654435761u + 1u; col8[r] = r * 0x9E3779B97F4A7C15ull + 3u; }
        const unsigned long long n4 = compact_column<uint32_t>(del.data(), col4.data(), count, 0u, out4.data());
        printf("L %llu", n4);
        for (uint32_t v : out4) printf(" %x", v);
        printf("\n");
        const unsigned long long n8 = compact_column<uint64_t>(del.data(), col8.data(), count, UINT64_MAX, out8.data());
        printf("K %llu", n8);
        for (uint64_t v : out8) printf(" %llx", (unsigned long long)v);
        printf("\n");
    }
    return 0;
}
'''


def COL4(n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(1)).astype(np.uint32)


def COL8(n):
    with np.errstate(over="ignore"):
        return np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)

SIZES = [0, 1, 31, 32, 33, 64, 100, 256, 1000, 1024, 4096, 5000]
CHUNKS = [32, 64, 96, 256, 1024]          # (the header's default, 65536 rows, is one case of its own below)
PATTERNS = ["none", "all", "prefix", "suffix", "alternate", "r1", "r50", "r99", "one_survivor", "row1"]


def tombstones(kind, n, rng):
    d = np.zeros(n, bool)
    if kind == "all":
        d[:] = True
    elif kind == "prefix":
        d[:n * 3 // 10] = True
    elif kind == "suffix":
        d[n - n * 3 // 10:] = True
    elif kind == "alternate":
        d[::2] = True
    elif kind in ("r1", "r50", "r99"):
        d = rng.random(n) < {"r1": 0.01, "r50": 0.5, "r99": 0.99}[kind]
    elif kind == "one_survivor":
        d[:] = True
        if n:
            d[rng.integers(n)] = False
    elif kind == "row1":
        if n > 1:
            d[1] = True
    return d


def pack(b, garbage_rng=None):
    """bool[n] -> uint32 words, bit i % 32 of word i / 32; the bits past n of the last word are garbage when asked."""
    n = b.size
    words = (n + 31) // 32
    full = np.zeros(words * 32, bool)
    full[:n] = b
    if garbage_rng is not None and words:
        full[n:] = garbage_rng.random(words * 32 - n) < 0.5
    return np.packbits(full, bitorder="little").view(np.uint32) if words else np.zeros(0, np.uint32)


def cases():
    rng = np.random.default_rng(7)
    out = []
    for n in SIZES:
        for chunk in CHUNKS:
            for kind in PATTERNS:
                out.append((n, chunk, 1000 if kind == "r50" else 0, kind, tombstones(kind, n, rng), rng.random(n) < 0.4))
    n = 3 * 65536 + 77                     # the default chunk
    out.append((n, 0, 5, "default/alternate", tombstones("alternate", n, rng), rng.random(n) < 0.4))
    out.append((n, 0, 0, "default/prefix", tombstones("prefix", n, rng), rng.random(n) < 0.4))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("compact_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    cs = cases()
    grng = np.random.default_rng(8)
    lines = []
    for n, chunk, offset, _, dead, allow in cs:
        lines.append(f"{n} {chunk} {offset}")
        lines.append(" ".join(f"{w:x}" for w in pack(dead, grng)))     # bits past the count must be ignored
        lines.append(" ".join(f"{w:x}" for w in pack(allow, grng)))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    res, i = [], 0
    for c in cs:
        live, first_moved, nch = (int(x) for x in out[i].split()[1:])
        chunks = [tuple(int(x) for x in out[i + 1 + j].split()[1:]) for j in range(nch)]
        i += 1 + nch
        base = np.array(out[i].split()[1:], dtype=np.uint64); i += 1
        ids = np.array([int(x) for x in out[i].split()[1:]], dtype=np.uint64); i += 1
        b = out[i].split()[1:]; i += 1
        cols = []
        for dt in (np.uint32, np.uint64):
            v = out[i].split()[1:]; i += 1
            cols.append((int(v[0]), np.array([int(x, 16) for x in v[1:]], dtype=dt)))
        res.append((c, live, first_moved, chunks, base, ids, int(b[0]), np.array([int(x, 16) for x in b[1:]], dtype=np.uint32), cols))
    assert i == len(out)
    return res


def test_chunks_read_every_live_row_once_and_write_densely(results):
    for (n, chunk, _, kind, dead, _), live, first_moved, chunks, *_ in results:
        what = (n, chunk, kind)
        chunk = chunk or 65536
        alive = ~dead
        before = np.concatenate([[0], np.cumsum(alive)])          # live rows below row i
        assert live == int(alive.sum()), what
        # rows below first_moved are live and stay; the first chunk starts at the first deleted row's word
        assert first_moved % 32 == 0 or first_moved == n, what
        assert alive[:first_moved].all(), what
        if dead.any():
            assert first_moved == int(np.argmax(dead)) // 32 * 32, what
        else:
            assert first_moved == n and not chunks, what
        # ascending, disjoint chunks of whole words; the rows between them are all deleted
        seen = np.zeros(n, np.int64)
        w_next = int(before[first_moved])
        r_next = first_moved
        for r0, r1, w0, L, staged in chunks:
            assert r0 % 32 == 0 and (r1 % 32 == 0 or r1 == n) and r_next <= r0 < r1 <= n, what
            assert not alive[r_next:r0].any(), what
            r_next = r1
            seen[r0:r1] += 1
            assert L == int(alive[r0:r1].sum()) and L > 0, what
            assert w0 == int(before[r0]) == w_next, what       # dense, order-preserving
            w_next = w0 + L
            assert w0 <= r0, what
            assert bool(staged) == (w0 + L > r0), what
            if staged:
                assert r1 - r0 <= chunk, what                       # one chunk fits the staging buffer
            assert w0 + L <= r1, what                               # never reaches a later chunk's source
        assert not alive[r_next:].any(), what
        assert w_next == live, what
        assert (seen[alive & (np.arange(n) >= first_moved)] == 1).all(), what


def test_no_destination_reaches_a_later_source(results):
    for (n, chunk, _, kind, _, _), _, _, chunks, *_ in results:
        for a in range(len(chunks)):
            for b in range(a + 1, min(len(chunks), a + 4)):
                assert chunks[a][2] + chunks[a][3] <= chunks[b][0], (n, chunk, kind, a, b)


def test_both_chunk_forms_occur(results):
    forms = {}
    for (n, chunk, _, kind, _, _), _, _, chunks, *_ in results:
        forms.setdefault(kind, set()).update(bool(c[4]) for c in chunks)
    assert forms["alternate"] == {True, False}       # staged at first, direct once the gap has opened
    assert forms["default/alternate"] == {True, False}
    assert forms["default/prefix"] == {False}        # a deleted prefix: all direct moves
    assert forms["suffix"] <= {True}                 # a deleted suffix: at most the one chunk that holds its start


def test_id_map_word_bases_and_bits_equal_numpy(results):
    for (n, chunk, offset, kind, dead, allow), live, _, _, base, ids, nsurv, out, _ in results:
        what = (n, chunk, kind)
        alive = ~dead
        want = np.full(n, ID_NONE, np.uint64)
        want[alive] = np.arange(live, dtype=np.uint64) + np.uint64(offset)
        assert np.array_equal(ids, want), what
        before = np.concatenate([[0], np.cumsum(alive)])
        assert np.array_equal(base, before[0:n:32].astype(np.uint64)), what
        assert nsurv == live, what
        words = (n + 31) // 32
        moved = np.zeros((words + 2) * 32, bool)
        moved[:live] = allow[alive]
        assert np.array_equal(out[:words + 2], np.packbits(moved, bitorder="little").view(np.uint32)), what
        assert out[words + 2] == 0xDEADBEEF, what     # nothing written past out_words


def test_columns_move_with_their_rows_and_the_tail_takes_the_default(results):
    for (n, chunk, _, kind, dead, _), live, *_, cols in results:
        what = (n, chunk, kind)
        for (nsurv, out), col, none, canary in ((cols[0], COL4(n), 0, 0xDEADBEEF), (cols[1], COL8(n), ID_NONE, 0xDEADBEEFDEADBEEF)):
            assert nsurv == live, what
            want = np.full(n, none, col.dtype)
            want[:live] = col[~dead]
            assert np.array_equal(out[:n], want), what
            assert out.size == n + 2 and (out[n:] == canary).all(), what     # nothing written past the count
