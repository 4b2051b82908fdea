"""The host-side plan of a diversified search (vrod_amd/csrc/diverse_plan.h), checked on the host: a small driver is
compiled with g++ against the real header (which therefore holds no HIP header).

  - the constants restate the ABI's limits;
  - diverse_check_args: k = 0, k > pool, pool > VROD_MAX_DIVERSE_POOL and a lambda that is NaN or outside [0, 1] are
    refused, in that order; the edges (k == pool, pool == the limit, lambda 0 and 1, -0.0) pass; the Python mirror the
    model carries decides the same;
  - the LDS arithmetic: at every dim in {1, 768, 4100, 32768} x pool in {1, 64, 1024} (and the limits around them) a
    work-group gets at least one wave and stays within 160 KB; the parts add up to what the kernel lays out; a wave per
    64 positions while they fit."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

import diverse_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
HDR = open(os.path.join(ROOT, "include", "vrod.h")).read()
MAX_POOL = int(re.search(r"#define VROD_MAX_DIVERSE_POOL (\d+)u", HDR).group(1))
MAX_DIM = int(re.search(r"#define VROD_MAX_DIM (\d+)u", HDR).group(1))
LDS_CAP = 160 * 1024
TILE = 64 * 68 * 4

DRIVER = r'''
#include <cstdio>
#include "diverse_plan.h"
using namespace vrod;

int main() {
    char what;
    printf("M %u %u %u %u %u %u\n", kDiverseMaxPool, kDiverseMaxDim, kDiverseLdsCap, kDiverseTileBytes, kDiverseMaxWaves, kDiverseFixedBytes);
    while (scanf(" %c", &what) == 1) {
        if (what == 'A') {
            unsigned k, pool; float lambda;
            scanf("%u %u %a", &k, &pool, &lambda);
            printf("A %d\n", diverse_check_args(k, pool, lambda));
        } else if (what == 'W') {
            unsigned dim, pool;
            scanf("%u %u", &dim, &pool);
            const unsigned w = diverse_waves(dim, pool);
            printf("W %u %u %u\n", w, diverse_lds_bytes(dim, pool, w), diverse_row_floats(dim));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("diverse_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_header_has_no_hip_and_constants_follow_the_abi(run):
    text = open(os.path.join(CSRC, "diverse_plan.h")).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
    m = run("")[0].split()
    assert m[:4] == ["M", str(MAX_POOL), str(MAX_DIM), str(LDS_CAP)]
    assert int(m[4]) == TILE and 1 <= int(m[5]) <= 16
    # the fixed part: the taken bits, a 64-bit key per wave, four control words
    assert int(m[6]) == MAX_POOL // 8 + int(m[5]) * 8 + 16
    assert DM.MAX_DIVERSE_POOL == MAX_POOL


def test_every_argument_check(run):
    nan, inf = float("nan"), float("inf")
    cases = [
        (0, 10, 0.5, 1), (0, 0, 0.5, 1), (0, 2000, nan, 1),                                   # k == 0 comes first
        (11, 10, 0.5, 2), (2, 1, 0.5, 2), (MAX_POOL + 1, MAX_POOL, 0.5, 2), (4000, 2000, 0.5, 2),   # then k > pool
        (10, MAX_POOL + 1, 0.5, 3), (MAX_POOL + 1, MAX_POOL + 1, 0.5, 3), (1, 0xFFFFFFFF, 0.5, 3),  # then the pool's limit
        (10, 10, nan, 4), (10, 10, -1e-9, 4), (10, 10, 1.0000001, 4), (10, 10, inf, 4), (10, 10, -inf, 4), (10, 10, 2.0, 4),
        (10, 10, 0.5, 0), (1, 1, 0.0, 0), (1, 1, 1.0, 0), (1, 1, -0.0, 0), (MAX_POOL, MAX_POOL, 0.3, 0), (1, MAX_POOL, 1.0, 0),
        (10, 100, 1e-45, 0), (10, 100, 0.99999994, 0),
    ]
    out = run("".join(f"A {k} {pool} {float(lam).hex() if lam == lam and abs(lam) != inf else lam}\n" for k, pool, lam, _ in cases))[1:]
    assert [int(x.split()[1]) for x in out] == [w for *_, w in cases]
    for k, pool, lam, want in cases:
        assert DM.check_args(k, pool, lam) == want, (k, pool, lam)


def test_lds_arithmetic_fits_at_every_shape(run):
    dims = [1, 2, 3, 4, 5, 63, 64, 100, 768, 4096, 4100, 20000, 32767, MAX_DIM]
    pools = [1, 2, 63, 64, 65, 100, 257, 512, 513, 1023, MAX_POOL]
    assert set([1, 768, 4100, 32768]) <= set(dims) and set([1, 64, 1024]) <= set(pools)
    grid = list(itertools.product(dims, pools))
    m = run("")[0].split()
    max_waves, fixed = int(m[5]), int(m[6])
    out = run("".join(f"W {d} {p}\n" for d, p in grid))[1:]
    for (d, p), line in zip(grid, out):
        w, lds, row = map(int, line.split()[1:])
        assert row == -(-d // 4) * 4 and row >= d
        assert 1 <= w <= max_waves, (d, p, w)
        assert lds <= LDS_CAP, (d, p, lds)
        assert lds == row * 4 + w * TILE + p * 12 + fixed
        want = min(max_waves, -(-p // 64))
        if w < want:   # fewer waves than positions ask for: only because one more tile would not fit
            assert lds + TILE > LDS_CAP, (d, p, w)
        else:
            assert w == want
    # the widest row with the largest pool still gets its wave; a narrow row gets all of them
    assert out[grid.index((MAX_DIM, MAX_POOL))].split()[1] == "1"
    assert int(out[grid.index((768, MAX_POOL))].split()[1]) == max_waves
    assert out[grid.index((768, 64))].split()[1] == "1" and out[grid.index((768, 65))].split()[1] == "2"
