"""The filter route of a search (vrod_amd/csrc/search_plan.h filter_route), checked on the host: a small driver is
compiled with g++ against the real header and prints its decisions over a grid of (dtype, forced path, N, m, nq, dim).

Rules: a forced GATHER path always gathers and a forced dense path (STREAM / MFMA / EXACT) never does; under AUTO the
gather path takes m = 0 and small filters and the dense scan takes m = N, and the choice is monotone -- a filter that
is dense at (m, nq) stays dense for every larger m and every larger nq."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")

AUTO, STREAM, MFMA, EXACT, GATHER = 0, 1, 2, 3, 4
F32, BF16 = 0, 1

DRIVER = r'''
#include <cstdio>
#include "search_plan.h"
using namespace vrod;

int main() {
    const unsigned long long Ns[] = {1, 1000, 300000, 10000000};
    const unsigned dims[] = {16, 128, 768, 1536};
    const unsigned nqs[] = {1, 2, 3, 4, 5, 8, 9, 16, 31, 32, 33, 64, 100, 256, 257, 512, 1000, 1024};
    for (int dtype = 0; dtype < 2; ++dtype)
    for (int forced = 0; forced < 5; ++forced)
    for (unsigned long long N : Ns)
    for (unsigned dim : dims)
    for (unsigned nq : nqs)
    for (int i = 0; i <= 64; ++i) {
        // m = 0, 1, then 64 steps up to N (the last one N itself)
        const unsigned long long m = i == 0 ? 0 : i == 1 ? 1 : N * (unsigned long long)(i - 1) / 63;
        printf("%d %d %llu %u %u %llu %d\n", dtype, forced, N, dim, nq, m, (int)filter_route(forced, dtype, N, m, nq, dim));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("filter_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        dtype, forced, N, dim, nq, m, g = (int(x) for x in line.split())
        rows[(dtype, forced, N, dim, nq, m)] = bool(g)
    return rows


def test_forced_paths_are_respected(table):
    for (dtype, forced, N, dim, nq, m), g in table.items():
        if forced == GATHER:
            assert g, (dtype, forced, N, dim, nq, m)
        elif forced in (STREAM, MFMA, EXACT):
            assert not g, (dtype, forced, N, dim, nq, m)


def test_auto_gathers_small_filters_and_scans_full_ones(table):
    for (dtype, forced, N, dim, nq, m), g in table.items():
        if forced != AUTO:
            continue
        if m == 0:
            assert g, ("m = 0 must gather", dtype, N, dim, nq)
        if m == N:
            assert not g, ("m = N must scan", dtype, N, dim, nq)
        if N >= 300000 and m * 10000 <= N:      # 0.01 % of a large corpus: gather for any batch
            assert g, ("0.01 % must gather", dtype, N, dim, nq, m)


def test_narrow_filter_of_a_full_batch_gathers(table):
    # the case the gather path exists for: 0.1 % of 10M rows, batch 1024 (and 4), d = 768
    steps = [m for (dt, f, N, dim, nq, m) in table if (dt, f, N, dim, nq) == (BF16, AUTO, 10000000, 768, 1024)]
    small = max(m for m in steps if m <= 10000)
    assert table[(BF16, AUTO, 10000000, 768, 1024, small)]
    assert table[(BF16, AUTO, 10000000, 768, 4, small)]
    # ... and a 10 % filter of a full batch costs what the dense scan costs: it scans
    big = min(m for m in steps if m >= 1000000)
    assert not table[(BF16, AUTO, 10000000, 768, 1024, big)]


def test_monotone_in_m(table):
    groups = {}
    for (dtype, forced, N, dim, nq, m), g in table.items():
        if forced == AUTO:
            groups.setdefault((dtype, N, dim, nq), []).append((m, g))
    for key, seq in groups.items():
        seq.sort()
        dense_seen = False
        for m, g in seq:
            if not g:
                dense_seen = True
            assert not (dense_seen and g), ("gather again after dense", key, m)


def test_monotone_in_nq(table):
    groups = {}
    for (dtype, forced, N, dim, nq, m), g in table.items():
        if forced == AUTO:
            groups.setdefault((dtype, N, dim, m), []).append((nq, g))
    for key, seq in groups.items():
        seq.sort()
        dense_seen = False
        for nq, g in seq:
            if not g:
                dense_seen = True
            assert not (dense_seen and g), ("gather again after dense", key, nq)
