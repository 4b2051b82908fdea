"""The host-side plan of near-duplicate detection (vrod_amd/csrc/near_plan.h), checked on the host: a small driver is
compiled with g++ against the real header, as test_dup_plan.py compiles dup_plan.h.

  - the flags: the diagnostic bit and nothing else;
  - the pool: the fixed budget, never fewer entries than eligible rows, exactly the eligible count under SMALL_POOL;
  - the batches: the graph's sizes, consecutive, in order, the last one partial, together the whole list;
  - the overflow rule: a total within the pool fits, a batch of several rows is split, a one-row batch cannot overflow;
  - the halving: two non-empty consecutive halves that are the batch, and repeated halving reaches every row once as a
    one-row batch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
BUDGET = 1 << 22

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "near_plan.h"
using namespace vrod;

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            printf("K %llu %x %u %u %u\n", (unsigned long long)kNearPoolBudget, kNearSmallPool, kNearErrWalk, kNearErrRetry, kNearErrRow);
        } else if (what == 'F') {
            unsigned flags;
            scanf("%x", &flags);
            printf("F %d\n", (int)near_flags_ok(flags));
        } else if (what == 'P') {
            unsigned long long elig; unsigned small;
            scanf("%llu %u", &elig, &small);
            printf("P %llu\n", (unsigned long long)near_pool_entries(elig, small != 0));
        } else if (what == 'B') {   // every batch of `elig` eligible rows
            unsigned long long elig; unsigned bf16;
            scanf("%llu %u", &elig, &bf16);
            const uint32_t batch = near_batch_rows(bf16 != 0, elig);
            const uint64_t nb = near_n_batches(elig, batch);
            printf("B %u %llu", batch, (unsigned long long)nb);
            for (uint64_t s = 0; s < nb; ++s) { const NearBatch b = near_batch(elig, batch, s); printf(" %llu:%u", (unsigned long long)b.first, b.rows); }
            printf("\n");
        } else if (what == 'V') {
            unsigned long long first, total, pool; unsigned rows;
            scanf("%llu %u %llu %llu", &first, &rows, &total, &pool);
            printf("V %d\n", (int)near_verdict(NearBatch{first, rows}, total, pool));
        } else if (what == 'H') {   // halve until one row is left everywhere, as the host flow's stack does: the leaves in order
            unsigned long long first; unsigned rows;
            scanf("%llu %u", &first, &rows);
            std::vector<NearBatch> todo{NearBatch{first, rows}};
            unsigned long long splits = 0;
            printf("H");
            while (!todo.empty()) {
                const NearBatch b = todo.back();
                todo.pop_back();
                if (near_verdict(b, 2, 1) == NEAR_SPLIT) {   // (a total over the pool: only the row count decides)
                    NearBatch lo, hi;
                    near_halves(b, &lo, &hi);
                    if (!lo.rows || !hi.rows || lo.first != b.first || hi.first != lo.first + lo.rows || lo.rows + hi.rows != b.rows || lo.rows < hi.rows) { printf(" BAD"); return 1; }
                    todo.push_back(hi);
                    todo.push_back(lo);
                    ++splits;
                } else {
                    printf(" %llu:%u", (unsigned long long)b.first, b.rows);
                }
            }
            printf(" | %llu\n", splits);
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("near_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_constants_are_the_source_s_and_the_abi_s(run):
    text = open(os.path.join(CSRC, "near_plan.h")).read()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    assert run("K\n") == [f"K {BUDGET} 80000000 1 2 4"]
    assert re.search(r"#define VROD_NEAR_SMALL_POOL 0x80000000u", header)
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only
    assert [run(f"F {f:x}\n")[0] for f in (0, 0x80000000, 1, 2, 0x40000000, 0x80000001, 0xFFFFFFFF)] == ["F 1", "F 1"] + ["F 0"] * 5


@pytest.mark.parametrize("elig", [1, 2, 255, 2500, BUDGET - 1, BUDGET, BUDGET + 1, 10_000_000, (1 << 32) - 256])
def test_pool_is_never_smaller_than_the_eligible_count(run, elig):
    pool = int(run(f"P {elig} 0\n")[0].split()[1])
    assert pool >= elig and pool >= BUDGET and pool == max(BUDGET, elig)         # the budget, unless one query could not fit
    assert int(run(f"P {elig} 1\n")[0].split()[1]) == elig                       # SMALL_POOL: exactly the eligible count
    # a one-row batch has at most `elig` hits: it fits either pool, so the halving always ends
    assert run(f"V 0 1 {elig} {pool}\n") == ["V 0"] and run(f"V 0 1 {elig} {elig}\n") == ["V 0"]


@pytest.mark.parametrize("bf16,size", [(1, 1024), (0, 256)])
@pytest.mark.parametrize("elig", [1, 255, 256, 257, 1024, 1025, 2500, 4096])
def test_batches_cover_the_list_in_order(run, bf16, size, elig):
    got = run(f"B {elig} {bf16}\n")[0].split()
    batch, nb = int(got[1]), int(got[2])
    pieces = [tuple(int(v) for v in g.split(":")) for g in got[3:]]
    assert batch == min(size, elig) and nb == -(-elig // batch) == len(pieces)
    at = 0
    for first, rows in pieces:
        assert first == at and 1 <= rows <= batch
        at += rows
    assert at == elig and all(rows == batch for _, rows in pieces[:-1])


def test_the_overflow_rule(run):
    assert run("V 0 256 2500 2500\n") == ["V 0"]                                 # a total of exactly the pool fits
    assert run("V 0 256 2501 2500\n") == ["V 1"] and run("V 768 2 2501 2500\n") == ["V 1"]
    assert run("V 5 1 2501 2500\n") == ["V 2"]                                   # cannot happen: one row, more hits than rows
    assert run("V 0 1024 0 0\n") == ["V 0"]


@pytest.mark.parametrize("first,rows", [(0, 1), (0, 2), (7, 3), (1024, 256), (0, 1024), (300, 1000), (2048, 452), (5, 37)])
def test_halving_covers_every_row_once_and_ends_at_one_row_batches(run, first, rows):
    leaves, splits = run(f"H {first} {rows}\n")[0][2:].split("|")
    leaves = [tuple(int(v) for v in g.split(":")) for g in leaves.split()]
    assert leaves == [(first + i, 1) for i in range(rows)]                       # every row once, in ascending order
    assert int(splits) == rows - 1                                               # a binary tree with `rows` leaves
