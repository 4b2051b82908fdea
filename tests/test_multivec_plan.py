"""The host-side plan of a multi-vector search (vrod_amd/csrc/multivec_plan.h), checked on the host: a small driver is
compiled with g++ against the real header.

  - the constants restate the ABI's limits;
  - multivec_check_lims: lims[0] != 0, a decreasing entry, an empty query and one with 257 vectors are refused;
  - multivec_first_k: the grouped search's rule; multivec_cut: whole queries, at most the batch's vectors, at least one;
  - multivec_certified: k candidates and a k-th S strictly better than U -- equal to U is NOT certified, fewer than k
    candidates are not, a NaN on either side is not, a short list (or one as long as the eligible rows) always is;
  - the Python mirror the GPU tests' model uses (tests/multivec_model.py) decides exactly as the header does."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

import multivec_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
HDR = open(os.path.join(ROOT, "include", "vrod.h")).read()
MAX_K = int(re.search(r"#define VROD_MAX_K (\d+)u", HDR).group(1))
MAX_VEC = int(re.search(r"#define VROD_MAX_QUERY_VECTORS (\d+)u", HDR).group(1))

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "multivec_plan.h"
using namespace vrod;

int main() {
    char what;
    printf("M %u %u %u %llu\n", kMultivecMaxK, kMultivecMaxVectors, kMultivecBatchVectors, (unsigned long long)kMultivecDenseShare);
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            unsigned k; unsigned long long e;
            scanf("%u %llu", &k, &e);
            printf("K %u\n", multivec_first_k(k, e));
        } else if (what == 'L' || what == 'U') {
            unsigned n, q0 = 0, maxv = 0;
            if (what == 'U') scanf("%u %u", &q0, &maxv);
            scanf("%u", &n);
            std::vector<uint32_t> lims(n);
            for (auto& v : lims) scanf("%u", &v);
            if (what == 'L') printf("L %d\n", multivec_check_lims(lims.data(), n - 1));
            else printf("U %u\n", maxv ? multivec_cut(lims.data(), n - 1, q0, maxv) : multivec_cut(lims.data(), n - 1, q0));
        } else if (what == 'C') {
            int any_short, higher; unsigned k1, nc, k; unsigned long long e; float kth, U;
            scanf("%d %u %llu %u %u %a %a %d", &any_short, &k1, &e, &nc, &k, &kth, &U, &higher);
            printf("C %d\n", multivec_certified(multivec_lists_complete(any_short, k1, e), nc, k, kth, U, higher) ? 1 : 0);
        } else if (what == 'B') {
            unsigned long long c, n;
            scanf("%llu %llu", &c, &n);
            printf("B %d\n", multivec_candidates_too_broad(c, n) ? 1 : 0);
        } else if (what == 'T') {
            unsigned e;
            scanf("%u", &e);
            printf("T %u\n", multivec_table_slots(e));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("multivec_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_constants_follow_the_abi_and_the_mirror(run):
    assert run("")[0].split() == ["M", str(MAX_K), str(MAX_VEC), str(MM.BATCH_VECTORS), str(MM.DENSE_SHARE)]
    assert (MM.MAX_K, MM.MAX_QUERY_VECTORS) == (MAX_K, MAX_VEC) and MM.BATCH_VECTORS >= MAX_VEC


def test_lims_checks(run):
    cases = [([0, 1], 0), ([0, 256], 0), ([0, 3, 4, 260], 0), ([1, 2], 1), ([0, 5, 4], 2), ([0, 0], 3), ([0, 2, 2, 3], 3),
             ([0, 257], 4), ([0, 1, 258], 4), ([0, 4, 3, 600], 2)]
    out = run("".join(f"L {len(l)} " + " ".join(map(str, l)) + "\n" for l, _ in cases))[1:]
    assert [int(x.split()[1]) for x in out] == [w for _, w in cases]


def test_first_k_is_the_grouped_rule(run):
    ks = [1, 2, 5, 10, 32, 33, 895, 896, 897, MAX_K - 1, MAX_K]
    es = [0, 1, 9, 33, 37, 42, 43, 7000, MAX_K, MAX_K + 1, 10_000_000, 1 << 33]
    grid = list(itertools.product(ks, es))
    out = run("".join(f"K {k} {e}\n" for k, e in grid))[1:]
    for (k, e), line in zip(grid, out):
        k1 = int(line.split()[1])
        assert k1 == min(MAX_K, e, max(4 * k, k + 32)) == MM.first_k(k, e), (k, e)
    assert MM.first_k(1, 7000) == 33 and MM.first_k(5, 7000) == 37 and MM.first_k(10, 7000) == 42


def test_cut_takes_whole_queries(run):
    lims = [0, 256, 512, 513, 2047, 2048, 2050, 2306, 4000, 4001]
    for maxv in (0, 256, 300, 2048):
        q0, cuts = 0, []
        while q0 < len(lims) - 1:
            q1 = int(run(f"U {q0} {maxv} {len(lims)} " + " ".join(map(str, lims)) + "\n")[1].split()[1])
            assert q1 == MM.cut(lims, q0, maxv or MM.BATCH_VECTORS)
            assert q1 > q0 and (q1 == q0 + 1 or lims[q1] - lims[q0] <= (maxv or MM.BATCH_VECTORS))
            if q1 < len(lims) - 1:   # (greedy: one more query would not fit)
                assert lims[q1 + 1] - lims[q0] > (maxv or MM.BATCH_VECTORS)
            cuts.append(q1)
            q0 = q1
        assert cuts[-1] == len(lims) - 1
    assert MM.cut([0, 2048, 2049], 0) == 1 and MM.cut([0, 2047, 2048, 2049], 0) == 2


def test_certificate(run):
    nan, inf = float("nan"), float("inf")
    nxt = float.fromhex("0x1.000002p+0")   # the fp32 value after 1.0
    cases = [
        # any_short, k1, eligible, candidates, k, kth, U, higher -> certified
        ((0, 37, 7000, 12, 5, nxt, 1.0, 1), 1),      # strictly better
        ((0, 37, 7000, 12, 5, 1.0, 1.0, 1), 0),      # equal to U: a non-candidate may tie and win by its label
        ((0, 37, 7000, 12, 5, 1.0, nxt, 1), 0),
        ((0, 37, 7000, 4, 5, 9.0, 1.0, 1), 0),       # fewer than k candidates, full lists
        ((1, 37, 7000, 4, 5, nan, nan, 1), 1),       # a short list: every label is a candidate
        ((1, 37, 7000, 12, 5, 1.0, 1.0, 1), 1),
        ((0, 37, 37, 4, 5, nan, 1.0, 1), 1),         # lists as long as the eligible rows
        ((0, 37, 38, 4, 5, nan, 1.0, 1), 0),
        ((0, 37, 7000, 12, 5, nan, 1.0, 1), 0),      # NaN certifies nothing
        ((0, 37, 7000, 12, 5, 1.0, nan, 1), 0),
        ((0, 37, 7000, 12, 5, inf, inf, 1), 0),
        ((0, 37, 7000, 12, 5, 1.0, nxt, 0), 1),      # L2: lower is better
        ((0, 37, 7000, 12, 5, 1.0, 1.0, 0), 0),
        ((0, 37, 7000, 12, 5, nxt, 1.0, 0), 0),
        ((0, 37, 7000, 12, 5, -0.0, 0.0, 1), 0),     # -0.0 == +0.0
    ]
    text = "".join("C %d %u %u %u %u %s %s %d\n" % (c[0], c[1], c[2], c[3], c[4], float(c[5]).hex(), float(c[6]).hex(), c[7]) for c, _ in cases)
    out = run(text)[1:]
    assert [int(l.split()[1]) for l in out] == [w for _, w in cases]
    for c, w in cases:
        assert MM.certified(MM.lists_complete(c[0], c[1], c[2]), c[3], c[4], c[5], c[6], bool(c[7])) == bool(w), c


def test_dense_share_and_table(run):
    cases = [(0, 7000), (1750, 7000), (1751, 7000), (7000, 7000), (1, 3), (1, 4), (2, 4)]
    out = run("".join(f"B {c} {n}\n" for c, n in cases))[1:]
    for (c, n), line in zip(cases, out):
        assert int(line.split()[1]) == int(c * MM.DENSE_SHARE > n) == int(MM.too_broad(c, n)), (c, n)
    for e in (1, 31, 32, 33, 1221, 256 * MAX_K):
        s = int(run(f"T {e}\n")[1].split()[1])
        assert s >= 2 * e and s >= 64 and s & (s - 1) == 0 and (s == 64 or s < 4 * e)
