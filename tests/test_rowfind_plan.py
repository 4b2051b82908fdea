"""The host-side plan of row lookup (vrod_amd/csrc/rowfind_plan.h), checked on the host: a small driver is compiled with
g++ against the real header, as test_dup_plan.py compiles dup_plan.h.

  - the lookup batches: the chunks of an add, or 96 rows under SMALL_BATCH; they tile the call exactly;
  - the batch table: find_duplicates' table for as many rows;
  - the resolution rule on small arrays: stored before the call, new in an earlier batch, repeated inside the batch, new."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
NONE = 0xFFFFFFFFFFFFFFFF

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "rowfind_plan.h"
using namespace vrod;

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            printf("K %x %x %llu %d %d %d\n", kRowfindNarrowHash, kRowfindSmallBatch, (unsigned long long)kRowfindSmallRows, (int)rowfind_flags_ok(0xC0000000u),
                   (int)rowfind_flags_ok(1u), (int)sizeof(RowfindAnswer));
        } else if (what == 'B') {   // B n dim small -> rows per batch, batches, then every batch's (first, count)
            unsigned long long n;
            unsigned dim, small;
            scanf("%llu %u %u", &n, &dim, &small);
            const uint64_t nb = rowfind_batches(n, dim, small != 0);
            printf("B %llu %llu %llu", (unsigned long long)rowfind_batch_rows(n, dim, small != 0), (unsigned long long)nb,
                   (unsigned long long)ingest_chunk_rows(n, dim));
            for (uint64_t b = 0; b <= nb && b < 8; ++b)
                printf(" %llu:%llu", (unsigned long long)rowfind_batch_first(n, dim, small != 0, b), (unsigned long long)rowfind_batch_count(n, dim, small != 0, b));
            printf("\n");
        } else if (what == 'S') {
            unsigned long long m;
            scanf("%llu", &m);
            printf("S %llu %llu\n", (unsigned long long)rowfind_table_slots(m), (unsigned long long)dup_table_slots(m));
        } else if (what == 'R') {   // R count0 id_offset append n batch, then n answers "row first" (row -1: none; first: index into its batch)
            unsigned long long count0, off, n, batch;
            unsigned append;
            scanf("%llu %llu %u %llu %llu", &count0, &off, &append, &n, &batch);
            std::vector<RowfindAnswer> ans(n);
            for (auto& a : ans) {
                long long row;
                unsigned long long first;
                scanf("%lld %llu", &row, &first);
                a.row = row < 0 ? kRowfindNone : (uint64_t)row;
                a.first = first;
            }
            std::vector<uint64_t> out(n, 7), fresh(n);
            std::vector<uint32_t> news(batch);
            RowfindTotals T;
            printf("R");
            for (uint64_t i0 = 0; i0 < n; i0 += batch) {
                const uint64_t m = n - i0 < batch ? n - i0 : batch;
                const uint64_t k = rowfind_resolve(ans.data() + i0, i0, m, count0, off, append != 0, out.data(), fresh.data(), news.data(), T);
                printf(" [");
                for (uint64_t j = 0; j < k; ++j) printf("%s%u", j ? "," : "", news[j]);
                printf("]");
            }
            printf(" |");
            for (uint64_t v : out) printf(" %lld", v == kRowfindNone ? -1ll : (long long)v);
            printf(" | %llu %llu %llu |", (unsigned long long)T.found, (unsigned long long)T.repeats, (unsigned long long)T.fresh);
            for (uint64_t j = 0; j < T.fresh; ++j) printf(" %llu", (unsigned long long)fresh[j]);
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
    d = tmp_path_factory.mktemp("rowfind_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_constants_are_the_abi_s(run):
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    text = open(os.path.join(CSRC, "rowfind_plan.h")).read()
    assert run("K\n") == ["K 80000000 40000000 96 1 0 16"]
    assert re.search(r"#define VROD_ROWFIND_NARROW_HASH 0x80000000u", header) and re.search(r"#define VROD_ROWFIND_SMALL_BATCH 0x40000000u", header)
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only
    assert "dup_word_term" not in text and "dup_mix" not in text and "0x9E37" not in text   # the hash is dup_plan.h's: nothing of it is restated


@pytest.mark.parametrize("n,dim,small", [(1, 8, 0), (150, 768, 0), (150, 768, 1), (96, 33, 1), (97, 33, 1), (2 * 96 + 5, 8, 1), (65536, 768, 0),
                                         (65537, 768, 0), (100_000, 768, 0), (5000, 32768, 0), (1_000_000, 8, 0), (95, 8, 1)])
def test_batches_tile_the_call(run, n, dim, small):
    got = run(f"B {n} {dim} {small}\n")[0].split()
    rows, nb, chunk = int(got[1]), int(got[2]), int(got[3])
    cuts = [tuple(int(v) for v in c.split(":")) for c in got[4:]]
    assert rows == (min(n, 96) if small else chunk) and nb == -(-n // rows)      # an add's chunks, or 96 rows
    if small:
        assert nb == -(-n // 96)
    if nb < 8:
        assert cuts[-1][1] == 0                                                  # the call is used up
        cuts = cuts[:-1]
        assert sum(c for _, c in cuts) == n
    pos = 0
    for first, count in cuts:
        assert first == pos and 0 < count <= rows
        pos += count
    assert all(c == rows for _, c in cuts[:-1])


@pytest.mark.parametrize("m", [1, 96, 255, 256, 257, 1024, 65536])
def test_table_is_find_duplicates_table(run, m):
    mine, dups = (int(v) for v in run(f"S {m}\n")[0].split()[1:])
    assert mine == dups and mine >= max(1024, 4 * m) and mine & (mine - 1) == 0


def resolve(run, count0, off, append, batch, answers):
    line = run(f"R {count0} {off} {int(append)} {len(answers)} {batch} " + " ".join(f"{r} {f}" for r, f in answers) + "\n")[0]
    lists, out, totals, fresh = line[2:].split("|")
    return (lists.split(), [int(v) for v in out.split()], tuple(int(v) for v in totals.split()), [int(v) for v in fresh.split()])


def test_resolution_rule_in_one_batch(run):
    # inputs: 0 stored (row 4), 1 new, 2 repeats 1, 3 stored (row 0), 4 new, 5 repeats 0's class (the device names the found row again)
    answers = [(4, 0), (-1, 1), (-1, 1), (0, 3), (-1, 4), (4, 0)]
    lists, out, totals, fresh = resolve(run, 10, 5000, False, 6, answers)
    assert lists == ["[1,4]"] and out == [5004, -1, -1, 5000, -1, 5004] and totals == (3, 1, 2) and fresh == [1, 4]
    lists, out, totals, fresh = resolve(run, 10, 5000, True, 6, answers)
    assert lists == ["[1,4]"] and out == [5004, 5010, 5010, 5000, 5011, 5004] and totals == (3, 1, 2) and fresh == [1, 4]


def test_resolution_rule_across_batches(run):
    # batches of 3.  Batch 0: new, stored, new.  Batch 1: the corpus (or the side corpus) now holds the call's new inputs as rows
    # count0 + 0 and count0 + 1: input 3 equals the second, input 4 is new, input 5 repeats 4.  Batch 2: input 6 equals input 4.
    answers = [(-1, 0), (2, 1), (-1, 2), (11, 0), (-1, 1), (-1, 1), (12, 0)]
    for append, want in ((True, [110, 102, 111, 111, 112, 112, 112]), (False, [-1, 102, -1, -1, -1, -1, -1])):
        lists, out, totals, fresh = resolve(run, 10, 100, append, 3, answers)
        assert lists == ["[0,2]", "[1]", "[]"] and out == want, (append, out)
        assert totals == (1, 3, 3) and fresh == [0, 2, 4]                        # found before the call; repeats; new
    # a row at or past count0 is never "found": found counts rows stored BEFORE the call
    _, out, totals, _ = resolve(run, 0, 0, True, 2, [(-1, 0), (-1, 0), (0, 0), (-1, 1)])
    assert out == [0, 0, 0, 1] and totals == (0, 2, 2)
