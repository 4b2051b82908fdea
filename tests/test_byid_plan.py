"""The host-side plan of vrod_knn_graph and vrod_search_by_ids (vrod_amd/csrc/byid_plan.h), checked on the host: a small
driver is compiled with g++ against the real header.

  - the batch cutting on a grid of (n, batch): every row of the range is covered exactly once and in order, only the
    last batch is partial, the slots alternate (two batches in flight never share a workspace);
  - the batch size by storage type, capped by the range, as the Python package restates it;
  - the search's k with and without the self drop, and the k limit that follows from it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
MAX_K = int(re.search(r"#define VROD_MAX_K (\d+)u", open(os.path.join(ROOT, "include", "vrod.h")).read()).group(1))

DRIVER = r'''
#include <cstdio>
#include "byid_plan.h"
using namespace vrod;

int main() {
    char what;
    printf("M %u %u %u\n", kByidMaxK, kByidBatchBf16, kByidBatchF32);
    while (scanf(" %c", &what) == 1) {
        if (what == 'B') {          // every batch of a range
            unsigned long long n; unsigned batch;
            scanf("%llu %u", &n, &batch);
            const uint64_t nb = byid_n_batches(n, batch);
            printf("B %llu", (unsigned long long)nb);
            for (uint64_t s = 0; s < nb; ++s) {
                const ByidBatch b = byid_batch(n, batch, s);
                printf(" %llu:%u:%u", (unsigned long long)b.first, b.rows, b.slot);
            }
            printf("\n");
        } else if (what == 'S') {   // batch size
            int bf16; unsigned long long n;
            scanf("%d %llu", &bf16, &n);
            printf("S %u\n", byid_batch_rows(bf16 != 0, n));
        } else {                    // k
            unsigned k; int ex;
            scanf("%u %d", &k, &ex);
            printf("K %u %d\n", byid_search_k(k, ex != 0), byid_k_ok(k, ex != 0) ? 1 : 0);
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("byid_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_constants_follow_the_abi_and_the_package(run):
    import vrod_amd
    out = run("")
    assert out[0].split() == ["M", str(MAX_K), str(vrod_amd.index.KNN_BATCH[vrod_amd.DTYPE_BF16]), str(vrod_amd.index.KNN_BATCH[vrod_amd.DTYPE_F32])]
    assert out[0].split()[2:] == ["1024", "256"]


def test_batches_cover_the_range_once_and_in_order(run):
    grid = []
    for batch in (1, 2, 7, 256, 1024):
        for n in sorted({0, 1, batch - 1, batch, batch + 1, 2 * batch + 300, 5 * batch}):
            if n >= 0:
                grid.append((n, batch))
    out = run("".join(f"B {n} {b}\n" for n, b in grid))[1:]
    assert len(out) == len(grid)
    for (n, batch), line in zip(grid, out):
        f = line.split()
        nb = int(f[1])
        parts = [tuple(int(x) for x in p.split(":")) for p in f[2:]]
        assert nb == len(parts) == -(-n // batch), (n, batch)
        at = 0
        for s, (first, rows, slot) in enumerate(parts):
            assert first == at and rows >= 1, (n, batch, s)       # in order, no gap, no overlap, no empty batch
            assert rows == batch or s == nb - 1, (n, batch, s)     # only the tail is partial
            assert slot == s % 2, (n, batch, s)                    # the slots alternate
            at += rows
        assert at == n, (n, batch)
        if nb:
            assert parts[-1][1] == n - (nb - 1) * batch


def test_batch_size_by_storage_type_and_range(run):
    cases = [(1, 1 << 20, 1024), (0, 1 << 20, 256), (1, 1024, 1024), (1, 1023, 1023), (0, 255, 255), (0, 256, 256), (1, 1, 1), (0, 1, 1),
             (1, 0, 1), (1, 1 << 33, 1024)]
    out = run("".join(f"S {b} {n}\n" for b, n, _ in cases))[1:]
    assert [int(l.split()[1]) for l in out] == [w for _, _, w in cases]


def test_search_k_and_its_limit(run):
    cases = [(1, 0, 1, 1), (1, 1, 2, 1), (10, 1, 11, 1), (MAX_K, 0, MAX_K, 1), (MAX_K - 1, 1, MAX_K, 1), (MAX_K, 1, MAX_K + 1, 0),
             (MAX_K + 1, 0, MAX_K + 1, 0), (0, 0, 0, 0), (0, 1, 1, 0)]
    out = run("".join(f"K {k} {e}\n" for k, e, _, _ in cases))[1:]
    assert [tuple(int(x) for x in l.split()[1:]) for l in out] == [(k1, ok) for _, _, k1, ok in cases]
