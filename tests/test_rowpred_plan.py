"""The host-side plan of the row-predicate operations (vrod_amd/csrc/rowpred_plan.h), checked on the host: a small driver
is compiled with g++ against the real header, as test_where_plan.py compiles where_plan.h.

  - the sizes: RowPred is 48 bytes with the label at 40, 1024 predicates of 52 bytes fit the 64 KiB LDS of a plain launch;
  - the pass cutting: 2048 rows per work-group, whole 64-row waves and exactly 64 hit words, the groups and the hit
    words of a count;
  - row_pred_matches and row_pred_unsatisfiable against their Python restatement (rowpred_model) on random and edge
    predicates: the sign boundary, the interval's ends, bit 63, label 0 and 0xFFFFFFFF, a label that is not compared;
  - row_pred_before: a strict order under which equal predicates, and only those, are neighbours."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rowpred_model import row_pred_matches
from where_model import I64_MAX, I64_MIN, unsatisfiable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")

DRIVER = r'''
#include <cstddef>
#include <cstdio>
#include "rowpred_plan.h"
using namespace vrod;

int main() {
    static_assert(sizeof(RowPred) == 48 && offsetof(RowPred, lo) == 24 && offsetof(RowPred, label) == 40 && offsetof(RowPred, has_label) == 44, "RowPred");
    static_assert(kRowPredsPerPass * kRowPredLdsPerPred <= 64 * 1024, "the pass's table fits the LDS of a plain launch");
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            printf("K %u %u %zu %u %u\n", kRowPredsPerPass, kRowPredLdsPerPred, sizeof(RowPred), kRowPredRowsPerGroup, kRowPredThreads);
        } else if (what == 'C') {
            unsigned long long n;
            scanf("%llu", &n);
            printf("C %u %llu\n", row_pred_groups(n), (unsigned long long)row_pred_hit_words(n));
        } else if (what == 'M') {
            unsigned long long t, a, b, c;
            long long v, lo, hi;
            unsigned l, label, has;
            scanf("%llx %lld %x %llx %llx %llx %lld %lld %x %u", &t, &v, &l, &a, &b, &c, &lo, &hi, &label, &has);
            const RowPred p{a, b, c, lo, hi, label, has};
            printf("M %d %d\n", (int)row_pred_matches(t, v, l, p), (int)row_pred_unsatisfiable(p));
        } else {
            unsigned long long a, b, c, a2, b2, c2;
            long long lo, hi, lo2, hi2;
            unsigned label, has, label2, has2;
            scanf("%llx %llx %llx %lld %lld %x %u %llx %llx %llx %lld %lld %x %u", &a, &b, &c, &lo, &hi, &label, &has, &a2, &b2, &c2, &lo2, &hi2,
                  &label2, &has2);
            printf("B %d\n", (int)row_pred_before(RowPred{a, b, c, lo, hi, label, has}, RowPred{a2, b2, c2, lo2, hi2, label2, has2}));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("rowpred_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_sizes_match_the_source_and_the_lds(run):
    text = open(os.path.join(CSRC, "rowpred_plan.h")).read()
    k = int(re.search(r"constexpr uint32_t kRowPredsPerPass = (\d+);", text).group(1))
    per = int(re.search(r"constexpr uint32_t kRowPredLdsPerPred = (\d+);", text).group(1))
    rows = int(re.search(r"constexpr uint32_t kRowPredRowsPerGroup = (\d+);", text).group(1))
    threads = int(re.search(r"constexpr uint32_t kRowPredThreads = (\d+);", text).group(1))
    assert run("K\n") == [f"K {k} {per} 48 {rows} {threads}"]
    assert k == 1024 and per == 48 + 4 and k * per == 52 * 1024 <= 64 * 1024
    assert rows == 2048 and rows % 64 == 0 and rows // 32 == 64                  # whole waves; a hit word per lane of one wave
    assert threads == 256 and rows % threads == 0
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only
    assert "1024 distinct predicates" in open(os.path.join(ROOT, "include", "vrod.h")).read()   # the header states the size


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 2048 + 37, 10_000_000, (1 << 32) - 256])
def test_pass_cutting(run, n):
    groups, words = (int(x) for x in run(f"C {n}\n")[0].split()[1:])
    assert groups == -(-n // 2048) and words == -(-n // 64) * 2
    assert words * 32 >= n and words <= max(groups, 0) * 64                      # every group's words lie within its 64


EDGE = [I64_MIN, I64_MIN + 1, -(1 << 32), -2, -1, 0, 1, 2, (1 << 31) - 1, 1 << 31, 1 << 32, I64_MAX - 1, I64_MAX]
LABELS = [0, 1, 7, 0x80000000, 0xFFFFFFFF]


def test_row_pred_matches_and_unsatisfiable(run):
    rng = np.random.default_rng(12)
    cases = []
    for _ in range(3000):
        v, lo, hi = (int(x) for x in rng.choice(EDGE, 3))
        if rng.random() < 0.3:
            v = int(rng.integers(I64_MIN, I64_MAX, endpoint=True))
        if rng.random() < 0.5:
            lo, hi = I64_MIN, I64_MAX
        t = int(rng.integers(0, 16)) | (int(rng.integers(0, 2)) << 63)
        a, b, c = (int(rng.integers(0, 16)) * int(rng.random() < 0.4) | (int(rng.random() < 0.15) << 63) for _ in range(3))
        l, label = (int(x) for x in rng.choice(LABELS, 2))
        cases.append((t, v, l, a, b, c, lo, hi, label, int(rng.random() < 0.5)))
    for l in LABELS:                                                             # the label decides, and only when it is compared
        for label in LABELS:
            cases += [(0, 0, l, 0, 0, 0, I64_MIN, I64_MAX, label, 1), (0, 0, l, 0, 0, 0, I64_MIN, I64_MAX, label, 0)]
    for v in EDGE:                                                               # both ends include a stored value
        cases += [(0, v, 7, 0, 0, 0, v, v, 7, 1), (0, v, 7, 0, 0, 0, I64_MIN, v, 7, 1), (0, v, 7, 0, 0, 0, v, I64_MAX, 1, 1)]
    out = run("".join("M %x %d %x %x %x %x %d %d %x %d\n" % c for c in cases))
    got = [tuple(int(x) for x in line.split()[1:]) for line in out]
    want = [(int(row_pred_matches(np.array([c[0]], np.uint64), np.array([c[1]], np.int64), np.array([c[2]], np.uint32), c[3:])[0]),
             int(unsatisfiable(c[3:8]))) for c in cases]
    assert got == want
    hits = [g[0] for g in got]
    assert 0.05 < sum(hits) / len(hits) < 0.95 and any(g[1] for g in got)
    assert all(not h for h, u in got if u)                                       # an unsatisfiable predicate matches no input
    assert got[3000:3000 + 2 * len(LABELS) ** 2] == [(int(l == label), 0) if has else (1, 0) for l in LABELS for label in LABELS for has in (1, 0)]


def test_row_pred_before_is_a_strict_order(run):
    preds = [(0, 0, 0, -1, 1, 0, 0), (0, 0, 0, -1, 1, 0, 1), (0, 0, 0, -1, 1, 7, 1), (0, 0, 0, -1, 1, 0xFFFFFFFF, 1), (0, 0, 0, I64_MIN, 1, 0, 0),
             (0, 0, 0, -1, I64_MAX, 0, 0), (1 << 63, 0, 0, -1, 1, 0, 0), (0, 1, 0, -1, 1, 0, 0), (0, 0, 1, -1, 1, 0, 0)]
    pairs = [(p, q) for p in preds for q in preds]
    out = run("".join("B %x %x %x %d %d %x %d %x %x %x %d %d %x %d\n" % (p + q) for p, q in pairs))
    before = {pq: int(line.split()[1]) for pq, line in zip(pairs, out)}
    for p in preds:
        assert not before[(p, p)]
        for q in preds:
            if p != q:
                assert before[(p, q)] + before[(q, p)] == 1                      # distinct predicates are ordered, one way
    key = lambda p: (p[0], p[1], p[2], p[3], p[4], p[6], p[5])                   # masks unsigned, ends signed, then the label
    for p, q in pairs:
        assert before[(p, q)] == int(key(p) < key(q))
