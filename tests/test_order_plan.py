"""The arithmetic of ordered selection (vrod_amd/csrc/order_plan.h), checked on the host: a small driver is compiled with
g++ against the real header, as test_rowpred_plan.py compiles rowpred_plan.h.

  - order_key is strictly monotone over the int64 edge values in both directions, and order_value inverts it;
  - order_after agrees with Python's tuple comparison on a grid of keys and ids;
  - order_pick on hand-made histograms: the rank in the first bucket, in the last, exactly on a bucket's edge, one past
    it, all mass in one bucket; and walking a key down all 8 rounds with order_digit / order_in_prefix finds the key of
    a given rank in a random multiset;
  - the geometry: the row-predicate passes' groups, the sort's sizes, the bitonic network sorting (key, id) records."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U64 = (1 << 64) - 1
EDGE = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX]

DRIVER = r'''
#include <cstdio>
#include <utility>
#include <vector>
#include "order_plan.h"
using namespace vrod;

int main() {
    static_assert(sizeof(OrderState) == 16, "OrderState");
    static_assert(kOrderSortTile * 16 <= 64 * 1024 && kOrderMaxRows % kOrderSortTile == 0, "a tile of records fits the LDS of a plain launch");
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'G') {
            printf("G %u %u %u %u %u %u %u\n", kOrderRounds, kOrderBins, kOrderThreads, kOrderChunksPerGroup, kOrderMaxRows, kOrderSortTile, kOrderSortThreads);
        } else if (what == 'K') {
            long long v;
            int desc;
            scanf("%lld %d", &v, &desc);
            const uint64_t k = order_key(v, desc);
            printf("K %llu %lld\n", (unsigned long long)k, (long long)order_value(k, desc));
        } else if (what == 'A') {
            unsigned long long k, i, ck, ci;
            scanf("%llu %llu %llu %llu", &k, &i, &ck, &ci);
            printf("A %d\n", (int)order_after(k, i, ck, ci));
        } else if (what == 'P') {   // remaining, then (bin, count) pairs up to -1
            unsigned remaining;
            int bin;
            uint32_t hist[kOrderBins] = {0};
            scanf("%u", &remaining);
            while (scanf("%d", &bin) == 1 && bin >= 0) scanf("%u", &hist[bin]);
            const OrderPick p = order_pick(hist, remaining);
            printf("P %u %u\n", p.digit, p.remaining);
        } else if (what == 'S') {   // rank, n, then n keys: the radix select as the kernels run it
            unsigned rank, n;
            scanf("%u %u", &rank, &n);
            std::vector<uint64_t> keys(n);
            for (auto& k : keys) { unsigned long long x; scanf("%llu", &x); k = x; }
            OrderState st{0, rank};
            for (uint32_t round = 0; round < kOrderRounds; ++round) {
                uint32_t hist[kOrderBins] = {0};
                for (uint64_t k : keys)
                    if (order_in_prefix(k, st.pivot, round)) ++hist[order_digit(k, round)];
                const OrderPick p = order_pick(hist, st.remaining);
                st.pivot |= (uint64_t)p.digit << (56u - 8u * round);
                st.remaining = p.remaining;
            }
            printf("S %llu %u\n", (unsigned long long)st.pivot, st.remaining);
        } else if (what == 'Z') {
            unsigned n;
            scanf("%u", &n);
            printf("Z %u %u\n", order_sort_size(n), order_groups(n));
        } else if (what == 'B') {   // n (key, id) records through the bitonic network over P slots, pads last
            unsigned n, P;
            scanf("%u %u", &n, &P);
            std::vector<std::pair<uint64_t, uint64_t>> r(P, {UINT64_MAX, UINT64_MAX});
            for (unsigned i = 0; i < n; ++i) { unsigned long long k, id; scanf("%llu %llu", &k, &id); r[i] = {k, id}; }
            for (uint32_t k = 2; k <= P; k <<= 1)
                for (uint32_t j = k / 2; j > 0; j >>= 1)
                    for (uint32_t t = 0; t < P / 2; ++t) {
                        const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
                        if (order_after(r[a].first, r[a].second, r[b].first, r[b].second) == order_bitonic_up(a, k)) std::swap(r[a], r[b]);
                    }
            for (unsigned i = 0; i < n; ++i) printf("B %llu %llu\n", (unsigned long long)r[i].first, (unsigned long long)r[i].second);
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("order_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_geometry_matches_the_source_and_the_header(run):
    text = open(os.path.join(CSRC, "order_plan.h")).read()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    assert run("G\n") == ["G 8 256 256 32 65536 2048 256"]
    assert int(re.search(r"#define VROD_MAX_ORDERED\s+(\d+)u", header).group(1)) == 65536
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only
    for n in (0, 1, 2047, 2048, 2049, 6151, 10_000_000):
        size, groups = (int(x) for x in run(f"Z {n}\n")[0].split()[1:])
        assert groups == -(-n // 2048)
        assert size >= max(n, 2048) and size & (size - 1) == 0 and (size == 2048 or size // 2 < n)
    assert run("Z 65536\n")[0].split()[1] == "65536"


def test_order_key_is_strictly_monotone_both_ways(run):
    for desc in (0, 1):
        out = [tuple(int(x) for x in line.split()[1:]) for line in run("".join(f"K {v} {desc}\n" for v in EDGE))]
        keys = [k for k, _ in out]
        assert [v for _, v in out] == EDGE                                       # order_value inverts order_key
        assert all(0 <= k <= U64 for k in keys)
        assert all(a > b for a, b in zip(keys, keys[1:])) if desc else all(a < b for a, b in zip(keys, keys[1:]))
    assert int(run(f"K {I64_MIN} 0\n")[0].split()[1]) == 0 and int(run(f"K {I64_MAX} 0\n")[0].split()[1]) == U64
    assert int(run(f"K {I64_MAX} 1\n")[0].split()[1]) == 0 and int(run(f"K {I64_MIN} 1\n")[0].split()[1]) == U64


def test_order_after_is_the_tuple_comparison(run):
    grid = [0, 1, 2, (1 << 63) - 1, 1 << 63, U64 - 1, U64]
    cases = [(k, i, ck, ci) for k in grid for i in grid for ck in grid for ci in grid]
    out = run("".join("A %d %d %d %d\n" % c for c in cases))
    assert [int(line.split()[1]) for line in out] == [int((k, i) > (ck, ci)) for k, i, ck, ci in cases]


def pick(run, remaining, hist):
    text = f"P {remaining} " + " ".join(f"{b} {c}" for b, c in hist.items()) + " -1\n"
    return tuple(int(x) for x in run(text)[0].split()[1:])


def test_order_pick_on_hand_made_histograms(run):
    h = {0: 5, 3: 4, 200: 1, 255: 10}                                            # cumulative: 5, 9, 10, 20
    assert pick(run, 1, h) == (0, 1) and pick(run, 5, h) == (0, 5)               # in the first bucket; exactly on its edge
    assert pick(run, 6, h) == (3, 1) and pick(run, 9, h) == (3, 4)               # one past the edge; the next edge
    assert pick(run, 10, h) == (200, 1)
    assert pick(run, 11, h) == (255, 1) and pick(run, 20, h) == (255, 10)        # in the last bucket, up to its last rank
    for b in (0, 7, 255):                                                        # all mass in one bucket: the rank is kept
        assert pick(run, 1, {b: 1000}) == (b, 1) and pick(run, 777, {b: 1000}) == (b, 777) and pick(run, 1000, {b: 1000}) == (b, 1000)
    assert pick(run, 3, {254: 2, 255: 2}) == (255, 1) and pick(run, 2, {254: 2, 255: 2}) == (254, 2)
    assert pick(run, 0xFFFFFFFF, {1: 0xFFFFFFFF}) == (1, 0xFFFFFFFF)


def test_eight_rounds_find_the_key_of_a_rank(run):
    rng = np.random.default_rng(5)
    sets = [rng.integers(0, 1 << 64, 500, dtype=np.uint64), rng.integers(0, 256, 500).astype(np.uint64), rng.integers(0, 256, 500).astype(np.uint64) << np.uint64(56),
            np.full(300, 1 << 63, np.uint64), np.array([0, U64, 1 << 63, (1 << 63) - 1] * 5, np.uint64)]
    for keys in sets:
        s = np.sort(keys)
        for rank in (1, 2, keys.size // 2, keys.size - 1, keys.size):
            pivot, rem = (int(x) for x in run(f"S {rank} {keys.size} " + " ".join(str(int(k)) for k in keys) + "\n")[0].split()[1:])
            below = int((keys < np.uint64(pivot)).sum())
            assert pivot == int(s[rank - 1]) and rem == rank - below and 1 <= rem <= int((keys == np.uint64(pivot)).sum())
    pivot, rem = (int(x) for x in run("S 64 300 " + " ".join([str(1 << 63)] * 300) + "\n")[0].split()[1:])
    assert (pivot, rem) == (1 << 63, 64)                                         # one tie class: pivot = that value, remainder = limit


def test_the_bitonic_network_sorts_records(run):
    rng = np.random.default_rng(6)
    for n, P in ((1, 2), (5, 8), (37, 64), (64, 64), (100, 128)):
        keys = rng.integers(0, 4, n).astype(np.uint64) * np.uint64(U64 // 3)     # heavy ties, both ends of the range
        ids = rng.permutation(n).astype(np.uint64) + np.uint64(U64 - n)          # unique, up to UINT64_MAX - 1
        out = run(f"B {n} {P} " + " ".join(f"{int(k)} {int(i)}" for k, i in zip(keys, ids)) + "\n")
        got = [tuple(int(x) for x in line.split()[1:]) for line in out]
        assert got == sorted(zip(keys.tolist(), ids.tolist()))
