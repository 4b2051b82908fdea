"""The host side of the row keys (vrod_amd/csrc/keys_plan.h), checked on the host: a small driver is compiled with g++
against the real header, as the other test_*_plan.py compile theirs.

  - the hash of a dozen fixed keys against its numpy restatement (keys_model.key_hash) and a second restatement in
    Python integers; the home slot is the hash's low bits;
  - the sizing rule at 0, 1, 255, 256, 257, 512, 513 live keys, and on growth from a table that exists (never smaller);
  - the load rule on a host rendering of insert and rebuild -- an open-addressing table with linear probing driven by
    the header's key_home, key_needs_rebuild and key_table_slots, the column deciding what a found slot is worth, as in
    kernels_keys.hip: 10 rounds of re-keying 300 rows keep occupied <= slots / 2, every current key is found, every
    old one is not, no walk runs over the table, and the bookkeeping model (keys_model.TableModel) agrees."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from keys_model import MIN_SLOTS, NONE, TableModel, home, key_hash, key_hash_int, keys_with_low_bits, table_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "keys_plan.h"
using namespace vrod;

// the table of kernels_keys.hip on the host, one thread: the same walks, bounded by the slot count
struct Table {
    std::vector<uint64_t> slot_key;
    std::vector<uint32_t> slot_row;
    uint64_t slots = 0, occupied = 0, rebuilds = 0, max_probe = 0;
    bool full = false;
    void clear(uint64_t n) {
        slots = key_table_slots(n, slots);
        slot_key.assign(slots, kKeyNone);
        slot_row.assign(slots, 0);
        occupied = 0; max_probe = 0;
    }
    void insert(uint64_t key, uint32_t row) {
        uint64_t s = key_home(key, slots), p = 0;
        for (; p < slots; ++p, s = (s + 1) & (slots - 1)) {
            if (slot_key[s] == kKeyNone) { slot_key[s] = key; ++occupied; }
            if (slot_key[s] == key) { slot_row[s] = row; break; }
        }
        if (p == slots) full = true;
        if (p + 1 > max_probe) max_probe = p + 1;
    }
    long long find(uint64_t key, const std::vector<uint64_t>& col) {
        uint64_t s = key_home(key, slots);
        for (uint64_t p = 0; p < slots; ++p, s = (s + 1) & (slots - 1)) {
            if (slot_key[s] == key) return col[slot_row[s]] == key ? (long long)slot_row[s] : -1;
            if (slot_key[s] == kKeyNone) return -1;
        }
        full = true;
        return -1;
    }
};

int main() {
    static_assert(kKeyNone == UINT64_MAX && kKeyMinSlots == 1024, "the contract's constants");
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'H') {
            unsigned long long k, slots;
            scanf("%llu %llu", &k, &slots);
            printf("H %llu %llu\n", (unsigned long long)key_hash(k), (unsigned long long)key_home(k, slots));
        } else if (what == 'S') {
            unsigned long long n, cur;
            scanf("%llu %llu", &n, &cur);
            printf("S %llu\n", (unsigned long long)key_table_slots(n, cur));
        } else if (what == 'N') {
            unsigned long long occ, inc, slots;
            scanf("%llu %llu %llu", &occ, &inc, &slots);
            printf("N %d\n", (int)key_needs_rebuild(occ, inc, slots));
        } else {   // 'R' rows rounds: every round gives every row a fresh key (round r, row i: r * 1000003 + i + 1)
            unsigned rows, rounds;
            scanf("%u %u", &rows, &rounds);
            Table T;
            std::vector<uint64_t> col(rows, kKeyNone);
            uint64_t keyed = 0;
            for (unsigned r = 0; r < rounds; ++r) {
                const bool first = T.slots == 0;
                const bool rebuild = first || key_needs_rebuild(T.occupied, rows, T.slots);
                const uint64_t sized_for = keyed + rows;
                for (unsigned i = 0; i < rows; ++i) col[i] = (uint64_t)r * 1000003ull + i + 1;
                keyed = rows;
                if (rebuild) { T.clear(sized_for); if (!first) T.rebuilds++; }
                for (unsigned i = 0; i < rows; ++i) T.insert(col[i], i);
                unsigned found = 0, ghosts = 0;
                for (unsigned i = 0; i < rows; ++i) found += T.find(col[i], col) == (long long)i;
                for (unsigned q = 0; q < r; ++q)
                    for (unsigned i = 0; i < rows; ++i) ghosts += T.find((uint64_t)q * 1000003ull + i + 1, col) >= 0;
                printf("R %llu %llu %llu %llu %u %u %d\n", (unsigned long long)T.slots, (unsigned long long)T.occupied,
                       (unsigned long long)T.rebuilds, (unsigned long long)T.max_probe, found, ghosts, (int)T.full);
            }
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("keys_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


FIXED = [0, 1, 2, 255, 1 << 31, (1 << 32) - 1, 1 << 32, 0x0123456789ABCDEF, 0x9E3779B97F4A7C15, (1 << 63), NONE - 1, NONE]


def test_the_header_is_host_arithmetic():
    text = open(os.path.join(CSRC, "keys_plan.h")).read()
    assert "hip/" not in text and "__global__" not in text


def test_hash_of_fixed_keys(run):
    out = run("".join(f"H {k} 4096\n" for k in FIXED))
    want = key_hash(np.array(FIXED, dtype=np.uint64))
    for k, line, w in zip(FIXED, out, want):
        assert line == f"H {int(w)} {int(w) & 4095}", k
        assert int(w) == key_hash_int(k), k
    assert np.array_equal(home(np.array(FIXED, np.uint64), 4096), want & np.uint64(4095))
    # the contract's worked example, by hand: key 0 is mix(golden)
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert int(want[0]) == z ^ (z >> 31)


def test_keys_with_chosen_low_bits(run):
    ks = keys_with_low_bits(5, 16, 0xFFFF)
    assert np.unique(ks).size == 5
    for slots in (1024, 2048, 65536):
        assert run("".join(f"H {int(k)} {slots}\n" for k in ks)) == [f"H {int(key_hash(np.uint64(k)))} {slots - 1}" for k in ks]


def test_sizing_rule(run):
    want = {0: 1024, 1: 1024, 255: 1024, 256: 1024, 257: 2048, 512: 2048, 513: 4096}
    for n, slots in want.items():
        assert run(f"S {n} 0\n") == [f"S {slots}"], n
        assert table_slots(n) == slots
        assert n <= slots // 4 and (slots == MIN_SLOTS or n > slots // 8)      # a quarter holds it, an eighth would not
    # growth: from a table that exists the rule only doubles, and keeps what is large enough
    for n, cur, slots in ((10, 4096, 4096), (1024, 4096, 4096), (1025, 4096, 8192), (600, 1024, 4096), (10_000_000, 1024, 1 << 26)):
        assert run(f"S {n} {cur}\n") == [f"S {slots}"], (n, cur)
        assert table_slots(n, cur) == slots
    # the load limit: one half, every incoming key counted as a new slot
    assert run("N 312 200 1024\nN 313 200 1024\nN 0 512 1024\nN 0 513 1024\n") == ["N 0", "N 1", "N 0", "N 1"]


def test_load_stays_at_most_one_half_under_rekeying(run):
    rows, rounds = 300, 10
    out = [[int(v) for v in line.split()[1:]] for line in run(f"R {rows} {rounds}\n")]
    assert len(out) == rounds
    model = TableModel()
    live = []
    rebuilds_seen = 0
    for r, (slots, occupied, rebuilds, max_probe, found, ghosts, full) in enumerate(out):
        new = [r * 1000003 + i + 1 for i in range(rows)]
        model.insert(len(live), new, new)
        live = new
        assert occupied <= slots // 2, (r, slots, occupied)
        assert (slots, occupied, rebuilds) == (model.slots, model.occupied, model.rebuilds), r
        assert found == rows and ghosts == 0 and not full, r
        assert 1 <= max_probe <= slots
        assert slots & (slots - 1) == 0 and slots >= MIN_SLOTS
        rebuilds_seen = rebuilds
    assert out[0][2] == 0 and rebuilds_seen >= 2          # the first table is no rebuild; stale slots force some later
