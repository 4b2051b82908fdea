"""The host-side plan of duplicate-row detection (vrod_amd/csrc/dup_plan.h), checked on the host: a small driver is
compiled with g++ against the real header, as test_rowpred_plan.py compiles rowpred_plan.h.

  - the table: a power of two of slots, at least 4 x live and at least 1024, and the smallest such;
  - the hash: it changes when two unequal elements swap places, when the last element changes and when the first does;
    it is the same for every split of the row's words into lane shares (a sum of per-word terms, then one finish); the
    label enters only under WITHIN_LABEL; the narrow form keeps 8 bits; the padding past dim never enters;
  - the read path: 16-byte units where dim * esize % 16 == 0, words with a tail mask otherwise, and the lanes per row."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "dup_plan.h"
using namespace vrod;

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            printf("K %u %u %llu %u\n", kDupRowsPerGroup, kDupThreads, (unsigned long long)kDupMinSlots, kDupEmpty);
        } else if (what == 'S') {
            unsigned long long live;
            scanf("%llu", &live);
            printf("S %llu\n", (unsigned long long)dup_table_slots(live));
        } else if (what == 'P') {
            unsigned dim, esize, ld;
            scanf("%u %u %u", &dim, &esize, &ld);
            const DupPlan p = dup_plan(dim, esize);
            printf("P %u %u %u %x %u %d %u\n", p.read, p.per_row, p.words, p.tail_mask, p.lanes, (int)dup_pitch_ok(dim, esize, ld), dup_groups(ld));
        } else if (what == 'H') {   // H dim esize label within narrow shares, then ceil(dim * esize / 4) words of the row in hex
            unsigned dim, esize, label, within, narrow, shares;
            scanf("%u %u %u %u %u %u", &dim, &esize, &label, &within, &narrow, &shares);
            const DupPlan p = dup_plan(dim, esize);
            std::vector<uint32_t> w(p.words + 4, 0xDEADBEEFu);   // what lies past the row must not matter
            for (unsigned i = 0; i < p.words; ++i) scanf("%x", &w[i]);
            const uint64_t whole = dup_row_hash(w.data(), dim, esize, label, within != 0, narrow != 0);
            // the same words dealt to `shares` lanes, lane l taking words l, l + shares, ...; the shares added in reverse
            std::vector<uint64_t> part(shares, 0);
            for (unsigned i = 0; i < p.words; ++i) part[i % shares] += dup_word_term(i + 1 == p.words ? w[i] & p.tail_mask : w[i], i);
            uint64_t sum = 0;
            for (unsigned l = shares; l-- > 0;) sum += part[l];
            printf("H %016llx %016llx %llu\n", (unsigned long long)whole, (unsigned long long)dup_finish(sum, label, within != 0, narrow != 0),
                   (unsigned long long)dup_home(whole, 4096));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("dup_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def row_words(row, dtype):
    """A row's stored bits as the 32-bit words the hash sums over: bf16 elements (given as uint16) two to a word, the last
    word of an odd dim zero-filled."""
    if dtype == "f32":
        return np.asarray(row, np.float32).view(np.uint32)
    e = np.asarray(row, np.uint16)
    if e.size % 2:
        e = np.append(e, np.uint16(0))
    return e.view(np.uint32)


def hash_line(row, dtype, label=0, within=0, narrow=0, shares=1):
    w = row_words(row, dtype)
    dim = len(row)
    return f"H {dim} {4 if dtype == 'f32' else 2} {label} {within} {narrow} {shares} " + " ".join("%x" % x for x in w) + "\n"


def hashes(run, lines):
    return [tuple(line.split()[1:]) for line in run("".join(lines))]


def test_constants_are_the_source_s(run):
    text = open(os.path.join(CSRC, "dup_plan.h")).read()
    rows = int(re.search(r"constexpr uint32_t kDupRowsPerGroup = (\d+);", text).group(1))
    threads = int(re.search(r"constexpr uint32_t kDupThreads = (\d+);", text).group(1))
    assert run("K\n") == [f"K {rows} {threads} 1024 {0xFFFFFFFF}"]
    assert rows == threads == 256 and rows % 64 == 0
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only


@pytest.mark.parametrize("live", [0, 1, 255, 256, 257, 1023, 1024, 1025, 256 + 37, 1_000_000, 10_000_000, (1 << 30) + 1, (1 << 32) - 256])
def test_slot_count(run, live):
    slots = int(run(f"S {live}\n")[0].split()[1])
    assert slots & (slots - 1) == 0 and slots >= 4 * live and slots >= 1024
    assert slots == 1024 or slots // 2 < 4 * live                                # and no larger than it has to be


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("dim", [8, 33, 768])
def test_hash_depends_on_position_and_on_every_element(run, dtype, dim):
    rng = np.random.default_rng(dim)
    if dtype == "f32":
        row = rng.standard_normal(dim).astype(np.float32)
        other = lambda v: np.float32(v + 1.0)
    else:
        row = rng.integers(1, 0x7F00, dim).astype(np.uint16)
        other = lambda v: np.uint16(v ^ 1)
    swapped, last, first, far = row.copy(), row.copy(), row.copy(), row.copy()
    swapped[[1, dim - 2]] = row[[dim - 2, 1]]
    assert row[1] != row[dim - 2]
    neighbours = row.copy()
    neighbours[[2, 3]] = row[[3, 2]]                                             # bf16: the two halves of one word
    assert row[2] != row[3]
    last[-1], first[0], far[dim // 2] = other(row[-1]), other(row[0]), other(row[dim // 2])
    got = hashes(run, [hash_line(r, dtype) for r in (row, row, swapped, neighbours, last, first, far)])
    whole = [g[0] for g in got]
    assert whole[0] == whole[1] and len(set(whole[1:])) == 6, whole
    assert all(g[0] == g[1] for g in got)                                        # one share: the definition itself


@pytest.mark.parametrize("dtype,dim", [("bf16", 8), ("bf16", 33), ("f32", 33), ("bf16", 768), ("f32", 768), ("bf16", 4099)])
def test_hash_is_the_same_for_every_split_into_lane_shares(run, dtype, dim):
    rng = np.random.default_rng(7 * dim)
    row = rng.standard_normal(dim).astype(np.float32) if dtype == "f32" else rng.integers(0, 0x10000, dim).astype(np.uint16)
    got = hashes(run, [hash_line(row, dtype, shares=s) for s in (1, 2, 3, 4, 16, 32, 64, 67)])
    assert len({g[0] for g in got}) == 1 and all(g[0] == g[1] for g in got), got


def test_label_narrow_form_and_padding(run):
    rng = np.random.default_rng(3)
    row = rng.integers(0, 0x10000, 33).astype(np.uint16)
    plain, lab0, lab7, lab7b, off7 = hashes(run, [hash_line(row, "bf16"), hash_line(row, "bf16", 0, 1), hash_line(row, "bf16", 7, 1),
                                                  hash_line(row, "bf16", 7, 1, shares=5), hash_line(row, "bf16", 7, 0)])
    assert off7[0] == plain[0]                                                   # without the flag the label is not read
    assert len({plain[0], lab0[0], lab7[0]}) == 3 and lab7[0] == lab7b[0] == lab7b[1]
    narrow = hashes(run, [hash_line(rng.integers(0, 0x10000, 33).astype(np.uint16), "bf16", narrow=1) for _ in range(400)])
    values = {int(g[0], 16) for g in narrow}
    assert max(values) < 256 and len(values) > 150                               # 8 bits are kept, and they are used
    # the home slot spreads them over the table: 200 values thrown at 4096 slots share about 200^2 / 8192 = 5 of them
    assert len({int(g[2]) for g in narrow}) >= len(values) - 20 and max(int(g[2]) for g in narrow) >= 2048
    assert all(0 <= int(g[2]) < 4096 for g in narrow)
    assert int(plain[0], 16) >= 1 << 32                                          # (the wide form is wide)
    # the upper half of an odd bf16 row's last word is padding: it never enters
    w = row_words(row, "bf16").copy()
    dirty = w.copy()
    dirty[-1] |= 0xABCD0000
    line = lambda ws: "H 33 2 0 0 0 1 " + " ".join("%x" % x for x in ws) + "\n"
    a, b = hashes(run, [line(w), line(dirty)])
    assert a[0] == b[0] == b[1]


@pytest.mark.parametrize("dim,esize,want", [
    (8, 2, (0, 1, 4, 0xFFFFFFFF, 1)), (8, 4, (0, 2, 8, 0xFFFFFFFF, 2)),
    (33, 2, (1, 17, 17, 0xFFFF, 32)), (33, 4, (1, 33, 33, 0xFFFFFFFF, 64)),
    (768, 2, (0, 96, 384, 0xFFFFFFFF, 64)), (768, 4, (0, 192, 768, 0xFFFFFFFF, 64)),
    (4099, 2, (1, 2050, 2050, 0xFFFF, 64)), (4099, 4, (1, 4099, 4099, 0xFFFFFFFF, 64)),
    (34, 2, (1, 17, 17, 0xFFFFFFFF, 32)), (1, 2, (1, 1, 1, 0xFFFF, 1)), (32768, 4, (0, 8192, 32768, 0xFFFFFFFF, 64)),
])
def test_read_path(run, dim, esize, want):
    ld = -(-dim // (64 if esize == 2 else 32)) * (64 if esize == 2 else 32)      # the handle's row pitch
    got = run(f"P {dim} {esize} {ld}\n")[0].split()[1:]
    read, per_row, words, tail, lanes, ok = int(got[0]), int(got[1]), int(got[2]), int(got[3], 16), int(got[4]), int(got[5])
    assert (read, per_row, words, tail, lanes) == want and ok == 1
    assert (read == 0) == (dim * esize % 16 == 0)
    assert lanes & (lanes - 1) == 0 and lanes <= 64 and (lanes >= per_row or lanes == 64) and (lanes == 1 or lanes // 2 < per_row)


def test_pitch_and_groups(run):
    assert run("P 33 2 64\n")[0].split()[6:] == ["1", "1"] and run("P 33 2 33\n")[0].split()[6] == "0"   # a pitch that breaks 16 bytes
    assert run("P 33 2 32\n")[0].split()[6] == "0"                               # a pitch below dim
    assert [int(run(f"P 8 2 {n}\n")[0].split()[7]) for n in (8, 256, 257, 293, 512, 513)] == [1, 1, 2, 2, 2, 3]   # (dup_groups of the third number)
