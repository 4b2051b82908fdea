"""The host-side plan of a grouped search (vrod_amd/csrc/group_plan.h), checked on the host: a small driver is compiled
with g++ against the real header.

  - group_first_k: k <= k1 <= VROD_MAX_K whenever there are at least k eligible rows, k1 = the eligible rows when they
    are fewer than the rule's value, never more than the rule's value, 0 without an eligible row;
  - group_resolved: a query is final with k labels, after a short list, or after a list as long as the eligible rows,
    and not otherwise;
  - the de-duplication kernel's table always keeps an empty slot and fits, with the labels beside it, 64 KB of LDS."""
import itertools
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
#include "group_plan.h"
using namespace vrod;

int main() {
    char what;
    printf("M %u %u\n", kGroupMaxK, kGroupDedupeMaxSlots);
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            unsigned k; unsigned long long e;
            scanf("%u %llu", &k, &e);
            const uint32_t k1 = group_first_k(k, e);
            printf("K %u %u %u\n", k1, group_dedupe_entries(k, k1), group_dedupe_slots(k, k1));
        } else {
            unsigned found, k, valid, k1; unsigned long long e;
            scanf("%u %u %u %u %llu", &found, &k, &valid, &k1, &e);
            printf("R %d\n", group_resolved(found, k, valid, k1, e) ? 1 : 0);
        }
    }
    return 0;
}
'''

KS = [1, 2, 3, 10, 31, 32, 33, 300, 895, 896, 897, 3551, 3552, 3553, MAX_K - 1, MAX_K]
ELIGIBLE = [0, 1, 2, 9, 10, 11, 33, 34, 42, 43, 299, 300, 1200, 1201, MAX_K - 1, MAX_K, MAX_K + 1, 20_000, 10_000_000, 1 << 33]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("group_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_constants_follow_the_abi(run):
    out = run("")
    assert out[0].split() == ["M", str(MAX_K), "8192"]


def test_first_k_on_a_grid(run):
    grid = list(itertools.product(KS, ELIGIBLE))
    out = run("".join(f"K {k} {e}\n" for k, e in grid))[1:]
    assert len(out) == len(grid)
    for (k, e), line in zip(grid, out):
        k1, entries, slots = (int(x) for x in line.split()[1:])
        rule = max(4 * k, k + 32)
        assert k1 == min(MAX_K, e, rule), (k, e, k1)
        if e >= k:
            assert k <= k1 <= MAX_K, (k, e, k1)
        if e < min(rule, MAX_K):
            assert k1 == e, (k, e, k1)
        # the kernel's LDS: the table never fills up, and table + labels stay within 64 KB (less the few static words)
        assert entries == k - 1 + k1 and entries < slots and slots & (slots - 1) == 0
        assert (slots + entries) * 4 <= 65536 - 64
        assert slots >= min(2 * entries, 8192)


def test_resolved_predicate(run):
    cases = [
        # found, k, valid, k1, eligible -> resolved
        ((10, 10, 42, 42, 20_000), 1),      # k labels
        ((12, 10, 42, 42, 20_000), 1),
        ((9, 10, 42, 42, 20_000), 0),       # a full list, fewer labels: rows below the list are unknown
        ((9, 10, 41, 42, 20_000), 1),       # a short list held every row that was left
        ((0, 10, 0, 42, 20_000), 1),        # ... an empty one too
        ((3, 10, 7, 7, 7), 1),              # a list as long as the eligible rows
        ((3, 10, 7, 7, 8), 0),
        ((1, 1, 33, 33, 1 << 33), 1),
        ((0, 1, 33, 33, 1 << 33), 0),
        ((3583, 3584, 3584, 3584, 10_000_000), 0),
    ]
    out = run("".join("R " + " ".join(str(x) for x in c) + "\n" for c, _ in cases))[1:]
    assert [int(l.split()[1]) for l in out] == [w for _, w in cases]
