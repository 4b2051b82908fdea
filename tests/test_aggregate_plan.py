"""The arithmetic of row aggregation (vrod_amd/csrc/aggregate_plan.h), checked on the host: a small driver is compiled
with g++ against the real header, as test_order_plan.py compiles order_plan.h.

  - agg_key: the label as it is, floor division on signed values over the int64 edges and random values and widths;
  - agg_home / agg_lds_home: the hash restated here (tests/test_gpu_aggregate.py builds its colliding labels from this
    restatement), the low bits for the global table, the bits from 32 up for the LDS table;
  - agg_table_slots at 0, 1, the floor, 2^20 and 2^20 + 1 rows, and the view's layout;
  - both comparators against Python's sort;
  - the constants the GPU test's patterns are built around."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import aggregate_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U64 = (1 << 64) - 1
LDS_SLOTS, LDS_PROBE, MIN_SLOTS, MAX_GROUPS = 512, 8, 1024, 1 << 20


def key_hash(key):
    """keys_plan.h key_hash (splitmix64's mixer over key + golden), all arithmetic mod 2^64."""
    z = (key + 0x9E3779B97F4A7C15) & U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
    return z ^ (z >> 31)


def home(key, slots):
    return key_hash(key & U64) & (slots - 1)


def lds_home(key, slots=LDS_SLOTS):
    return (key_hash(key & U64) >> 32) & (slots - 1)


def table_slots(count):
    s = MIN_SLOTS
    while s < 2 * min(count, MAX_GROUPS):
        s *= 2
    return s


DRIVER = r'''
#include <cstdio>
#include <algorithm>
#include <vector>
#include "aggregate_plan.h"
using namespace vrod;

int main() {
    static_assert(sizeof(AggGroup) == 48 && sizeof(AggCounters) == 32, "six and four 64-bit words");
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'G') {
            printf("G %u %u %u %u %u %u %u %u %llu %u %lld %llu\n", kAggByLabel, kAggByValue, kAggByTag, kAggOrderCount, kAggMaxGroups, kAggTagGroups,
                   kAggLdsSlots, kAggLdsProbe, (unsigned long long)kAggMinSlots, kAggThreads, (long long)kAggEmptyKey, (unsigned long long)kAggNoId);
        } else if (what == 'K') {
            unsigned by, label;
            long long v, w;
            scanf("%u %u %lld %lld", &by, &label, &v, &w);
            printf("K %lld\n", (long long)agg_key(by, label, v, w));
        } else if (what == 'H') {
            long long key;
            unsigned long long slots;
            scanf("%lld %llu", &key, &slots);
            printf("H %llu %u %llu\n", (unsigned long long)agg_home(key, slots), agg_lds_home(key, kAggLdsSlots), (unsigned long long)key_hash((uint64_t)key));
        } else if (what == 'Z') {
            unsigned long long n;
            scanf("%llu", &n);
            const uint64_t slots = agg_table_slots(n);
            std::vector<char> block(agg_table_bytes(8));
            const AggTable t = agg_table_view(block.data(), 8);
            const bool packed = (char*)t.ctr == block.data() && (char*)t.key == block.data() + 32 && (char*)t.count == (char*)t.key + 72 &&
                                (char*)t.min_value == (char*)t.count + 72 && (char*)t.max_value == (char*)t.min_value + 72 &&
                                (char*)t.sum_value == (char*)t.max_value + 72 && (char*)t.first_id == (char*)t.sum_value + 72 &&
                                (char*)(t.first_id + 9) == block.data() + block.size() && t.slots == 8;
            printf("Z %llu %llu %u %d\n", (unsigned long long)slots, (unsigned long long)agg_table_bytes(slots), agg_groups(n), (int)packed);
        } else if (what == 'C') {   // order, n, then n (key, count) pairs: the groups sorted by the plan's comparator
            unsigned by_count, n;
            scanf("%u %u", &by_count, &n);
            std::vector<AggGroup> g(n);
            for (auto& x : g) { long long k; unsigned long long c; scanf("%lld %llu", &k, &c); x = AggGroup{k, c, 0, 0, 0, 0}; }
            std::sort(g.begin(), g.end(), by_count ? agg_before_count : agg_before_key);
            for (auto& x : g) printf("C %lld %llu\n", (long long)x.key, (unsigned long long)x.count);
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("aggregate_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_constants_match_the_source_and_the_header(run):
    text = open(os.path.join(CSRC, "aggregate_plan.h")).read()
    header = open(os.path.join(ROOT, "include", "vrod.h")).read()
    assert run("G\n") == [f"G 0 1 2 4 {MAX_GROUPS} 64 {LDS_SLOTS} {LDS_PROBE} {MIN_SLOTS} 256 {I64_MIN} {U64}"]
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only
    for name, value in (("VROD_AGG_BY_LABEL", 0), ("VROD_AGG_BY_VALUE", 1), ("VROD_AGG_BY_TAG", 2), ("VROD_AGG_ORDER_COUNT", 4), ("VROD_MAX_AGG_GROUPS", MAX_GROUPS)):
        assert int(re.search(r"#define %s\s+(\d+)u" % name, header).group(1)) == value
    assert LDS_SLOTS & (LDS_SLOTS - 1) == 0 and (LDS_SLOTS + 1) * 48 <= 32 * 1024 and LDS_PROBE < LDS_SLOTS


def test_keys(run):
    rng = np.random.default_rng(11)
    edge = [I64_MIN, I64_MIN + 1, -86401, -86400, -86399, -11, -10, -9, -2, -1, 0, 1, 2, 9, 10, 11, 86399, 86400, I64_MAX - 1, I64_MAX]
    values = edge + rng.integers(I64_MIN, I64_MAX, 200, endpoint=True).tolist() + rng.integers(-10**6, 10**6, 200).tolist()
    widths = [1, 2, 3, 10, 86400, (1 << 62) + 1, I64_MAX - 1, I64_MAX] + rng.integers(1, I64_MAX, 20, endpoint=True).tolist()
    cases = [(v, w) for v in values for w in widths]
    out = run("".join(f"K 1 77 {v} {w}\n" for v, w in cases))
    assert [int(x.split()[1]) for x in out] == [v // w for v, w in cases]          # Python's // floors
    assert -1 // 10 == -1 and int(run("K 1 0 -1 10\n")[0].split()[1]) == -1
    for v in (I64_MIN, -1, 0, I64_MAX):                                          # width 1: the value itself
        assert int(run(f"K 1 0 {v} 1\n")[0].split()[1]) == v
    labels = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    out = run("".join(f"K 0 {lab} -5 0\n" for lab in labels))                      # the label, never sign-extended; value and width unread
    assert [int(x.split()[1]) for x in out] == labels


def test_home_slots_are_the_restated_hash(run):
    rng = np.random.default_rng(12)
    keys = [I64_MIN + 1, -1, 0, 1, I64_MAX, 0xFFFFFFFF] + rng.integers(I64_MIN + 1, I64_MAX, 100, endpoint=True).tolist() + list(range(40))
    for slots in (MIN_SLOTS, 4096, 1 << 21):
        out = [tuple(int(x) for x in line.split()[1:]) for line in run("".join(f"H {k} {slots}\n" for k in keys))]
        assert out == [(home(k, slots), lds_home(k), key_hash(k & U64)) for k in keys]
    # the numpy restatement the GPU test builds its patterns from is the same function
    arr = np.array(keys, np.int64)
    assert AM.key_hash(arr).tolist() == [key_hash(k & U64) for k in keys] and AM.lds_home(arr).tolist() == [lds_home(k) for k in keys]
    assert AM.home(arr, 4096).tolist() == [home(k, 4096) for k in keys]
    assert (AM.LDS_SLOTS, AM.LDS_PROBE, AM.MIN_SLOTS, AM.MAX_AGG_GROUPS) == (LDS_SLOTS, LDS_PROBE, MIN_SLOTS, MAX_GROUPS)
    assert len(set(AM.lds_home(np.arange(8192)).tolist())) == LDS_SLOTS          # small labels reach every LDS slot
    both = AM.labels_sharing_both_homes(LDS_PROBE + 4, MIN_SLOTS, like=5)        # enough to overrun the LDS probe
    assert both[0] == 5 and len(set(both.tolist())) == LDS_PROBE + 4
    assert {lds_home(int(k)) for k in both} == {lds_home(5)} and {home(int(k), MIN_SLOTS) for k in both} == {home(5, MIN_SLOTS)}


def test_table_sizes(run):
    for n in (0, 1, MIN_SLOTS // 2, MIN_SLOTS // 2 + 1, MIN_SLOTS, 4097, MAX_GROUPS - 1, MAX_GROUPS, MAX_GROUPS + 1, 10_000_000):
        slots, nbytes, groups, packed = (int(x) for x in run(f"Z {n}\n")[0].split()[1:])
        assert slots == table_slots(n) == AM.table_slots(n) and slots & (slots - 1) == 0 and slots >= max(MIN_SLOTS, 2 * min(n, MAX_GROUPS))
        assert slots == MIN_SLOTS or slots // 2 < 2 * min(n, MAX_GROUPS)          # the smallest such power of two
        assert nbytes == 32 + (slots + 1) * 48 and groups == -(-n // 2048) and packed == 1
    assert table_slots(0) == table_slots(MIN_SLOTS // 2) == MIN_SLOTS and table_slots(MIN_SLOTS // 2 + 1) == 2 * MIN_SLOTS
    assert table_slots(MAX_GROUPS) == table_slots(MAX_GROUPS + 1) == table_slots(10**9) == 1 << 21


def test_both_comparators(run):
    rng = np.random.default_rng(13)
    keys = rng.permutation(np.concatenate([[I64_MIN, -1, 0, 1, I64_MAX], rng.integers(I64_MIN, I64_MAX, 60)])).tolist()   # unique
    assert len(set(keys)) == len(keys)
    counts = rng.integers(1, 4, len(keys)).tolist()
    counts[0], counts[1] = U64, 1 << 63                                          # counts are unsigned
    text = " ".join(f"{k} {c}" for k, c in zip(keys, counts))
    got = [tuple(int(x) for x in line.split()[1:]) for line in run(f"C 0 {len(keys)} {text}\n")]
    assert got == sorted(zip(keys, counts))
    got = [tuple(int(x) for x in line.split()[1:]) for line in run(f"C 1 {len(keys)} {text}\n")]
    assert got == sorted(zip(keys, counts), key=lambda kc: (-kc[1], kc[0]))
