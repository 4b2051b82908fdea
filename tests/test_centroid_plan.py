"""The arithmetic of group centroids (vrod_amd/csrc/centroid_plan.h), checked on the host: a small driver is compiled
with g++ against the real header, as test_aggregate_plan.py compiles aggregate_plan.h, and every function is compared
with tests/centroid_model.py, the numpy restatement of the definition:

  - centroid_row_bits at the powers of two, centroid_exponent at each exponent boundary, centroid_scale;
  - centroid_quantise -- integer arithmetic in the header, llrint(double(x) * 2^s) in the model -- on subnormals, -0.0,
    the largest finite fp32, exact ties on both sides of zero, every shift from far left to far right, random bits;
  - centroid_sum_value and centroid_mean_value on sums that need 62 bits, on ties of the int64 -> fp64 rounding, on
    results that are fp32 subnormals and on S == 0;
  - the workspace view and the team geometry."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import centroid_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")

DRIVER = r'''
#include <cstdio>
#include <cstring>
#include <vector>
#include "centroid_plan.h"
using namespace vrod;

int main() {
    static_assert(sizeof(CentroidGroup) == 24, "three 64-bit words");
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'G') {
            printf("G %u %u %u %u %u %u %d\n", kCentroidSum, kCentroidMaxGroups, kCentroidNonFinite, kCentroidNoRank, kCentroidThreads, kCentroidInFlight,
                   kCentroidCosineExponent);
        } else if (what == 'R') {
            unsigned long long n;
            scanf("%llu", &n);
            printf("R %d\n", centroid_row_bits(n));
        } else if (what == 'E') {
            unsigned m;
            int R;
            scanf("%u %d", &m, &R);
            printf("E %d %d\n", centroid_exponent(m), centroid_scale(R, centroid_exponent(m)));
        } else if (what == 'Q') {
            unsigned bits;
            int s;
            scanf("%u %d", &bits, &s);
            printf("Q %lld\n", (long long)centroid_quantise(bits, s));
        } else if (what == 'O') {
            long long S;
            unsigned long long count;
            int s;
            scanf("%lld %llu %d", &S, &count, &s);
            const float a = centroid_sum_value(S, s), b = centroid_mean_value(S, count, s);
            unsigned ua, ub;
            memcpy(&ua, &a, 4);
            memcpy(&ub, &b, 4);
            printf("O %u %u\n", ua, ub);
        } else if (what == 'W') {
            unsigned long long groups, slots;
            scanf("%llu %llu", &groups, &slots);
            std::vector<char> block(centroid_ws_bytes(groups, slots));
            const CentroidWs w = centroid_ws_view(block.data(), groups);
            const bool packed = (char*)w.max_bits == block.data() && (char*)w.keys == block.data() + 8 && (char*)w.counts == (char*)(w.keys + groups) &&
                                (char*)w.rank == (char*)(w.counts + groups) && (char*)(w.rank + slots + 1) == block.data() + block.size();
            printf("W %d %llu\n", (int)packed, (unsigned long long)centroid_acc_bytes(groups, 768));
        } else if (what == 'T') {
            unsigned dim, esize;
            scanf("%u %u", &dim, &esize);
            const unsigned per = centroid_elems_per_piece(esize), pieces = centroid_pieces(dim, per);
            printf("T %u %u %u\n", per, pieces, centroid_team(pieces));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("centroid_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_constants_match_the_source_and_the_header(run):
    text = open(os.path.join(CSRC, "centroid_plan.h")).read()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    assert run("G\n") == [f"G 8 65536 {0x7F800000} {0xFFFFFFFF} 256 4 1"]
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only
    for name, value in (("VROD_CENTROID_SUM", 8), ("VROD_MAX_CENTROID_GROUPS", 65536)):
        assert int(re.search(r"#define %s\s+(\d+)u" % name, header).group(1)) == value
    assert (CM.CENTROID_SUM, CM.MAX_CENTROID_GROUPS, CM.NON_FINITE) == (8, 65536, 0x7F800000)


def test_row_bits_exponent_and_scale(run):
    ns = [0, 1, 2, 3, 4, 4095, 4096, 4097, (1 << 32) - 1, 1 << 32, (1 << 40) + 5]
    assert run("".join(f"R {n}\n" for n in ns)) == [f"R {CM.row_bits(n)}" for n in ns]
    ms = [0, 1, 0x007FFFFF, 0x00800000, 0x00FFFFFF, 0x01000000, 0x3F7FFFFF, 0x3F800000, 0x3FFFFFFF, 0x40000000, 0x7F000000, 0x7F7FFFFF]
    ms += [e << 23 for e in range(255)] + [(e << 23) - 1 for e in range(1, 256)]   # m at each exponent boundary, and just below it
    for R in (1, 13, 24):
        n = (1 << R) - 1
        assert run("".join(f"E {m} {R}\n" for m in ms)) == [f"E {CM.exponent(m)} {CM.scale(n, CM.exponent(m))}" for m in ms]


def test_quantiser_equals_llrint_of_the_exact_product(run):
    rng = np.random.default_rng(7)
    cases = []
    # ties: m24 * 2^sh with the dropped bits exactly a half, odd and even floors, both signs; sh from far left to far right
    for e in (0, 1, 2, 100, 127, 150, 200, 254):
        for mant in (0, 1, 2, 3, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF, 0x000800, 0x001800, 0x000801):
            for sign in (0, 1):
                bits = (sign << 31) | (e << 23) | mant
                E = CM.exponent(bits & 0x7FFFFFFF)
                for R in (1, 13, 30):
                    cases.append((bits, 62 - R - E))                             # the scale at which this element is the largest
                    cases.append((bits, 62 - R - min(E + 20, 128)))              # ... and 2^20 below the largest
                    cases.append((bits, 62 - R - min(E + 40, 128)))              # ... and lost below the quantum
    specials = [0.0, -0.0, 1.401298464324817e-45, -1.401298464324817e-45, 1.1754942106924411e-38, 1.1754943508222875e-38, 3.4028234663852886e38,
                -3.4028234663852886e38, 1.0, -1.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.99999994, 1e30, 1e-30]
    for x in specials:
        for s in (-66, -40, -1, 0, 1, 23, 24, 25, 41, 49, 60, 149, 150, 186):
            cases.append((f32_bits(x), s))
    for bits in rng.integers(0, 1 << 32, 3000, dtype=np.uint64):
        bits = int(bits)
        if (bits & 0x7F800000) == 0x7F800000:
            continue
        E = CM.exponent(bits & 0x7FFFFFFF)
        cases.append((bits, 62 - int(rng.integers(1, 34)) - min(E + int(rng.integers(0, 30)), 128)))
    # only scales at which the element fits: |x| < 2^E' with s = 62 - R - E' and R >= 1, as every call guarantees
    cases = [(b, s) for b, s in cases if max((b >> 23) & 0xFF, 1) - 126 + s <= 61]
    got = run("".join(f"Q {b} {s}\n" for b, s in cases))
    x = np.array([b for b, _ in cases], np.uint32).view(np.float32)
    for i, (b, s) in enumerate(cases):
        want = int(CM.quantise(x[i:i + 1], s)[0])
        assert got[i] == f"Q {want}", f"bits {b:#x} s {s}: {got[i]} != {want}"
    assert len(cases) > 4000


def test_output_conversions(run):
    rng = np.random.default_rng(8)
    cases = [(0, 1, 49), (0, 7, -60), (1, 1, 49), (-1, 3, 49), ((1 << 62) - 1, 4095, 49), (-(1 << 62) + 1, 4095, -78), ((1 << 62) - 1, 1, -66),
             ((1 << 53) + 1, 1, 20), ((1 << 53) + 3, 1, 20), ((1 << 54) + 2, 3, 20), ((1 << 54) + 6, 1, 20),   # ties of int64 -> fp64
             (3, 2, 149), (1, 2, 149), (5, 4, 150), (1, 3, 186), (-7, 2, 186), (12345, 7, 160),                # fp32 subnormal results
             ((1 << 24) + 1, 1, 24), ((1 << 25) + 2, 2, 24), ((1 << 24) + 1, 3, 0)]                            # ties of fp64 -> fp32
    for _ in range(2000):
        bits = int(rng.integers(1, 62))
        S = int(rng.integers(-(1 << bits), 1 << bits))
        cases.append((S, int(rng.integers(1, 1 << int(rng.integers(1, 30)))), int(rng.integers(-66, 187))))
    got = run("".join(f"O {S} {c} {s}\n" for S, c, s in cases))
    for i, (S, c, s) in enumerate(cases):
        a = int(CM.sum_value(np.array([S], np.int64), s).view(np.uint32)[0])
        b = int(CM.mean_value(np.array([S], np.int64), np.array([c], np.uint64), s).view(np.uint32)[0])
        assert got[i] == f"O {a} {b}", f"S {S} count {c} s {s}: {got[i]} != {a} {b}"
    assert run("O 0 5 49\n") == ["O 0 0"]                                        # +0.0f


def test_workspace_and_geometry(run):
    assert run("W 1 1024\nW 5000 16384\nW 65536 2097152\n") == [f"W 1 {768 * 8}", f"W 1 {5000 * 768 * 8}", f"W 1 {65536 * 768 * 8}"]
    want = {(1, 2): (8, 1, 1), (3, 2): (8, 1, 1), (8, 2): (8, 1, 1), (9, 2): (8, 2, 2), (200, 2): (8, 25, 32), (768, 2): (8, 96, 128), (1030, 2): (8, 129, 256),
            (4096, 2): (8, 512, 256), (1, 4): (4, 1, 1), (3, 4): (4, 1, 1), (8, 4): (4, 2, 2), (200, 4): (4, 50, 64), (768, 4): (4, 192, 256),
            (1030, 4): (4, 258, 256), (32768, 4): (4, 8192, 256)}
    assert run("".join(f"T {d} {e}\n" for d, e in want)) == [f"T {p} {n} {t}" for p, n, t in want.values()]
