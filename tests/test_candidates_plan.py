"""The host-side plan of the candidate-list searches (vrod_amd/csrc/candidates_plan.h), checked on the host: a small driver
is compiled with g++ against the real header.

  - the constants restate the ABI and the Python package;
  - lims arrays that do not start at 0 or that decrease, and the length cap at 16384 / 16385 entries;
  - the sort network of a list: the next power of two, for lengths 0, 1, 2, 3, 64, 65 and 16384, and the launch class it
    puts the query into (a short list never sits in the work-group of a long one);
  - the slot tables of a batch with empty lists in it: one slot and one segment per query that has a row;
  - the tiles of the ragged score launch, and the query a block finds for itself."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
HDR = open(os.path.join(ROOT, "include", "vrod.h")).read()
MAX_CAND = int(re.search(r"#define VROD_MAX_CANDIDATES (\d+)u", HDR).group(1))

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "candidates_plan.h"
using namespace vrod;

static std::vector<uint32_t> read_words(unsigned n) {
    std::vector<uint32_t> v(n);
    for (unsigned i = 0; i < n; ++i) scanf("%u", &v[i]);
    return v;
}

int main() {
    char what;
    printf("M %u %u", kCandMaxList, kCandClasses);
    for (unsigned c = 0; c < kCandClasses; ++c) printf(" %u %u", kCandClassCap[c], kCandClassThreads[c]);
    printf("\n");
    while (scanf(" %c", &what) == 1) {
        if (what == 'N') {          // one length: its network and its class
            unsigned len;
            scanf("%u", &len);
            printf("N %u %u\n", cand_network_size(len), cand_sort_class(len));
        } else if (what == 'L') {   // a lims array
            unsigned nq;
            scanf("%u", &nq);
            std::vector<uint32_t> l = read_words(nq + 1);
            uint32_t bad = 0;
            const int rc = cand_check_lims(l.data(), nq, &bad);
            printf("L %d %u\n", rc, rc == 2 ? bad : 0u);
        } else if (what == 'S') {   // the sort plan of a batch
            unsigned nq;
            scanf("%u", &nq);
            std::vector<uint32_t> l = read_words(nq + 1);
            const CandSortPlan P = cand_sort_plan(l.data(), nq);
            printf("S");
            for (unsigned c = 0; c <= kCandClasses; ++c) printf(" %u", P.first[c]);
            printf(" |");
            for (uint32_t q : P.order) printf(" %u", q);
            printf("\n");
        } else if (what == 'T') {   // the slot tables: lims, then the resolved lengths
            unsigned nq;
            scanf("%u", &nq);
            std::vector<uint32_t> l = read_words(nq + 1), len = read_words(nq);
            const CandSlots S = cand_slot_tables(l.data(), len.data(), nq);
            printf("T %u %u %llu %u |", S.n_empty, S.max_len, (unsigned long long)S.rows, S.T.size());
            for (uint32_t s = 0; s < S.T.size(); ++s) printf(" %u:%u:%u", S.T.slot_q[s], S.T.slot_len[s], S.T.slot_base[s]);
            printf(" |");
            for (const SegGroup& g : S.T.segs) printf(" %u:%u:%u:%u", g.list_base, g.m, g.slot0, g.nq);
            const SegPlan P = plan_segments(S.T.segs);
            printf(" | %zu %zu\n", P.entries.size(), P.chunks.size());
        } else {                    // 'O': tile offsets, and the query of every block
            unsigned nq;
            scanf("%u", &nq);
            std::vector<uint32_t> l = read_words(nq + 1);
            const std::vector<uint32_t> off = cand_tile_offsets(l.data(), nq);
            printf("O");
            for (uint32_t o : off) printf(" %u", o);
            printf(" |");
            for (uint32_t b = 0; b < off[nq]; ++b) printf(" %u", cand_tile_query(off.data(), nq, b));
            printf("\n");
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("candidates_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def words(run, what, lims, extra=()):
    line = f"{what} {len(lims) - 1} " + " ".join(map(str, list(lims) + list(extra)))
    out = run(line + "\n")[1]
    assert out[0] == what
    return out[1:].strip()


def test_constants_follow_the_abi_and_the_package(run):
    import vrod_amd
    head = run("")[0].split()
    assert head[:3] == ["M", str(MAX_CAND), "3"]
    assert MAX_CAND == 16384 and MAX_CAND * 4 == 64 * 1024        # one list of 32-bit rows is the work-group's 64 KB of LDS
    assert vrod_amd.index.MAX_CANDIDATES == MAX_CAND
    caps, threads = [int(x) for x in head[3::2]], [int(x) for x in head[4::2]]
    assert caps == sorted(caps) and caps[-1] == MAX_CAND
    # a thread of the sort owns whole 16-byte units of its class's capacity, at most 16 entries
    assert all(c % t == 0 and (c // t) % 4 == 0 and c // t <= 16 and t % 64 == 0 and t <= 1024 for c, t in zip(caps, threads))


def test_lims_validation_and_the_length_cap(run):
    assert words(run, "L", [0, 0, 3, 3, 10]) == "0 0"
    assert words(run, "L", [0]) == "0 0"
    assert words(run, "L", [1, 2]) == "1 0"                          # does not start at 0
    assert words(run, "L", [0, 5, 4]) == "1 0"                       # decreases
    assert words(run, "L", [0, 16384]) == "0 0"
    assert words(run, "L", [0, 16385]) == "2 0"
    assert words(run, "L", [0, 7, 7 + 16384, 7 + 16384 + 16385, 40000]) == "2 2"
    assert words(run, "L", [0, 16384, 32768, 49152]) == "0 0"        # the cap is per list, not per batch
    assert words(run, "L", [0, 0xFFFFFFFF]) == "2 0"
    assert words(run, "L", [0, 20000, 10]) == "1 0"                  # a malformed array is reported as such first


def test_network_size_and_launch_class(run):
    cases = {0: 0, 1: 1, 2: 2, 3: 4, 64: 64, 65: 128, 16384: 16384, 8193: 16384, 8192: 8192, 4097: 8192, 257: 512, 256: 256}
    out = run("".join(f"N {n}\n" for n in cases))[1:]
    got = [tuple(int(x) for x in l.split()[1:]) for l in out]
    assert [g[0] for g in got] == list(cases.values())
    # the class: networks of up to 256, up to 4096, up to 16384 entries
    assert [g[1] for g in got] == [0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 1, 0]


def test_sort_plan_groups_the_queries_by_class(run):
    # lengths 3, 5000, 0, 300, 16384, 256
    lims = [0, 3, 5003, 5003, 5303, 21687, 21943]
    assert words(run, "S", lims) == "0 3 4 6 | 0 2 5 3 1 4"
    assert words(run, "S", [0]) == "0 0 0 0 |"


def test_slot_tables_of_a_batch_with_empty_lists(run):
    # five queries, lists of 4, 0, 6, 2, 3 entries; resolved to 3, 0, 0, 2, 1 rows
    lims = [0, 4, 4, 10, 12, 15]
    out = words(run, "T", lims, [3, 0, 0, 2, 1])
    head, slots, segs, plan = [p.strip() for p in out.split("|")]
    assert head == "2 3 6 3"                                         # two empty queries, longest 3, six rows, three slots
    assert slots == "0:3:0 3:2:10 4:1:12"                            # slot_q : slot_len : slot_base = lims[q]
    assert segs == "0:3:0:1 10:2:1:1 12:1:2:1"                       # one segment of one query per slot
    assert plan == "3 1"                                             # three table entries, one launch
    # nothing resolved at all: no slot, no launch
    out = words(run, "T", [0, 2, 4], [0, 0])
    assert [p.strip() for p in out.split("|")] == ["2 0 0 0", "", "", "0 0"]


def test_tiles_of_the_score_launch(run):
    # lists of 1, 0, 64, 65, 130 entries: 1, 0, 1, 2, 3 tiles
    lims = [0, 1, 1, 65, 130, 260]
    off, owner = [p.strip() for p in words(run, "O", lims).split("|")]
    assert off == "0 1 1 2 4 7"
    assert owner == "0 2 3 3 4 4 4"
    off, owner = [p.strip() for p in words(run, "O", [0, 0, 0, 5]).split("|")]
    assert off == "0 0 0 1" and owner == "2"
