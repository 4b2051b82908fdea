"""The host decisions of a range search (vrod_amd/csrc/search_plan.h), compiled with g++ as tests/test_search_plan.py
does: the split policy of the filtered launches (range_split) and the widening of the caller's threshold into the fast
pass's threshold (range_fast_threshold), on values worked out by hand."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
CAP, TILE = 8192, 256

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "search_plan.h"
using namespace vrod;
static float from_bits(const char* s) { uint32_t u = (uint32_t)strtoul(s, 0, 16); float f; memcpy(&f, &u, 4); return f; }
int main(int argc, char** argv) {
    if (!strcmp(argv[1], "split")) {        // lo hi max_count cap -> bounds
        for (uint64_t b : range_split(strtoull(argv[2], 0, 10), strtoull(argv[3], 0, 10), strtoull(argv[4], 0, 10), (uint32_t)atoi(argv[5])))
            printf("%llu ", (unsigned long long)b);
        printf("\n");
    } else if (!strcmp(argv[1], "thr")) {   // thr_bits form eps_mode c_bits qn2_bits xn2_bits -> bits canonical
        bool canon = false;
        const float t = range_fast_threshold(from_bits(argv[2]), atoi(argv[3]), atoi(argv[4]), from_bits(argv[5]), from_bits(argv[6]), from_bits(argv[7]), &canon);
        uint32_t u; memcpy(&u, &t, 4);
        printf("%08x %d\n", u, (int)canon);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not CXX:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("range_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    r = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True).stdout.split()
    return run


def f32(x):
    return np.float32(x)


def hexbits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def unbits(h):
    return np.float32(struct.unpack("<f", struct.pack("<I", int(h, 16)))[0])


# ---------------------------------------------------------------- range_split
@pytest.mark.parametrize("lo, hi, max_count", [(0, 1_000_000, 8193), (0, 1_000_000, 20000), (0, 10_000_000, 5_000_000), (512, 1300, 9000),
                                                (0, 700, 100000), (256 * 40, 256 * 41 + 7, 50000), (0, 2 ** 32 - 256, 2 ** 32 - 256)])
def test_pieces_are_tile_aligned_and_cover_the_range_once(driver, lo, hi, max_count):
    b = [int(x) for x in driver("split", lo, hi, max_count, CAP)]
    assert b[0] == lo and b[-1] == hi
    assert all(x < y for x, y in zip(b, b[1:])), b                     # no empty piece, each row once
    assert all(x % TILE == 0 for x in b[1:-1]), b                      # inner bounds on tile boundaries
    tiles = -(-hi // TILE) - lo // TILE
    want = min(tiles, max(2, -(-max_count // (CAP // 2))))
    assert len(b) - 1 == want, (b, want)


def test_piece_counts_for_given_overflows(driver):
    n = lambda mc, hi=10_000_000: len(driver("split", 0, hi, mc, CAP)) - 1
    assert n(CAP) == 1                 # a full list is not an overflow
    assert n(CAP + 1) == 3             # ceil(8193 / 4096)
    assert n(2 * CAP) == 4
    assert n(20000) == 5
    assert n(10 ** 9) == 10_000_000 // TILE + 1   # never more pieces than tiles (39063 of them)
    assert n(100, hi=10_000) == 1      # nothing overflowed: nothing to split


def test_a_single_tile_is_never_split(driver):
    assert driver("split", 0, 256, 10 ** 6, CAP) == ["0", "256"]
    assert driver("split", 1024, 1100, 10 ** 6, CAP) == ["1024", "1100"]
    assert driver("split", 0, 257, 10 ** 6, CAP) == ["0", "256", "257"]   # two tiles: one piece each


# ---------------------------------------------------------------- range_fast_threshold
U = f32(2.0 ** -24)
DENORM = f32(2.3509887e-38)


def eps_of(mode, c, qn2, xn2):
    """The header's expression in fp32, step by step."""
    qn, xn = np.sqrt(f32(qn2)), np.sqrt(f32(xn2))
    span = f32(qn * xn) if mode == 0 else f32(f32(qn + xn) * f32(qn + xn))
    return f32(f32(f32(c) * span) + f32(f32(c) * DENORM)), span


@pytest.mark.parametrize("form, mode, dim, qn2, xn2, thr", [
    (0, 0, 768, 1.0, 1.0, 0.5), (0, 0, 768, 1.0, 1.0, -0.25), (0, 0, 96, 4.0, 9.0, 0.0), (0, 0, 768, 1.0, 1.0, 1e-30),
    (1, 2, 768, 1.0, 1.0, 1.5), (1, 2, 96, 100.0, 400.0, 0.0), (1, 2, 768, 1.0, 1.0, -3.0)])
def test_threshold_moves_by_eps_and_one_float_further(driver, form, mode, dim, qn2, xn2, thr):
    c = f32(f32(4.0) * f32(dim if mode == 0 else dim + 4) * U)
    eps, _ = eps_of(mode, c, qn2, xn2)
    out, canon = driver("thr", hexbits(thr), form, mode, hexbits(c), hexbits(qn2), hexbits(xn2))
    t = unbits(out)
    moved = f32(f32(thr) - eps) if form == 0 else f32(f32(thr) + eps)
    want = np.nextafter(moved, f32(-np.inf) if form == 0 else f32(np.inf))
    assert canon == "0" and t == want and hexbits(t) == hexbits(want)
    # the superset property in exact arithmetic: strictly on the worse side of threshold -/+ eps
    exact = float(f32(thr)) - float(eps) if form == 0 else float(f32(thr)) + float(eps)
    assert float(t) < exact if form == 0 else float(t) > exact


def test_hand_computed_values(driver):
    # dot form, c = 2^-10, |q| = |x| = 1, threshold 1: eps = 2^-10 (+ a denormal that rounds away); 1 - 2^-10 is a float,
    # one float below it is 1 - 2^-10 - 2^-24
    out, canon = driver("thr", hexbits(1.0), 0, 0, hexbits(2.0 ** -10), hexbits(1.0), hexbits(1.0))
    assert canon == "0" and float(unbits(out)) == 1.0 - 2.0 ** -10 - 2.0 ** -24
    # L2 through the norm expansion, c = 2^-10, |q| = |x| = 1: span = 4, eps = 2^-8; 2 + 2^-8 -> one float above: + 2^-22
    out, canon = driver("thr", hexbits(2.0), 1, 2, hexbits(2.0 ** -10), hexbits(1.0), hexbits(1.0))
    assert canon == "0" and float(unbits(out)) == 2.0 + 2.0 ** -8 + 2.0 ** -22
    # zero norms: eps is the denormal slack alone, c * 2^-125
    out, canon = driver("thr", hexbits(0.0), 0, 0, hexbits(2.0 ** -10), hexbits(0.0), hexbits(0.0))
    assert canon == "0" and float(unbits(out)) == float(np.nextafter(f32(-f32(2.0 ** -10) * DENORM), f32(-np.inf)))


@pytest.mark.parametrize("form, mode", [(0, 0), (1, 2)])
def test_infinite_thresholds_stay_infinite(driver, form, mode):
    c = hexbits(2.0 ** -10)
    for thr in (np.inf, -np.inf):
        out, canon = driver("thr", hexbits(thr), form, mode, c, hexbits(1.0), hexbits(1.0))
        assert canon == "0" and out == hexbits(thr)


@pytest.mark.parametrize("form, mode, qn2, xn2", [(0, 0, 3.4e38, 3.4e38), (0, 0, np.inf, 1.0), (0, 0, np.nan, 1.0), (1, 2, 3e38, 3e38),
                                                   (1, 2, 1.0, np.inf), (1, 1, 1.0, 1.0), (0, 0, 0.0, np.inf)])
def test_no_finite_bound_means_the_canonical_route(driver, form, mode, qn2, xn2):
    out, canon = driver("thr", hexbits(0.5), form, mode, hexbits(2.0 ** -10), hexbits(qn2), hexbits(xn2))
    assert canon == "1"
    assert out == hexbits(np.inf if form == 0 else -np.inf)   # and the fast pass appends nothing for it
