"""The host-side plan of a labelled search (vrod_amd/csrc/label_plan.h), checked on the host: a small driver is compiled
with g++ against the real header.

  - label_groups: the distinct labels ascending, every query in exactly one group, ascending within its group;
  - plan_segments + seg_lookup (the function the score kernel calls per block): over all blocks of all chunks, every
    (score slot, 64-row tile) pair of every group is covered exactly once, a block's queries stay inside its entry, a
    short last subgroup covers only its own queries, consecutive blocks of one tile are neighbours, every slot belongs
    to exactly one chunk and a chunk's score block respects the byte limit (groups of fewer than 8 queries aside);
  - SlotTables::add, which builds those groups and the per-slot arrays of a pass: a group's slot0 is the running slot
    count, slot_len / slot_base repeat its m / list_base once per query, slot_q lists its queries in the order given,
    and the groups it built pass the coverage checks above."""
import itertools
import os
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
#include "label_plan.h"
using namespace vrod;

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'G') {
            unsigned nq;
            scanf("%u", &nq);
            std::vector<uint32_t> l(nq + 1);
            for (unsigned i = 0; i < nq; ++i) scanf("%u", &l[i]);
            const LabelGroups g = label_groups(l.data(), nq);
            printf("G %u\n", g.size());
            for (uint32_t i = 0; i < g.size(); ++i) {
                printf("L %u", g.labels[i]);
                for (uint32_t j = g.q_off[i]; j < g.q_off[i + 1]; ++j) printf(" %u", g.q_order[j]);
                printf("\n");
            }
        } else {
            unsigned ng;
            unsigned long long limit;
            scanf("%u %llu", &ng, &limit);
            std::vector<SegGroup> gs(ng);
            uint32_t slot = 0, base = 0;
            if (what == 'T') {   // the groups through SlotTables::add, each with its queries
                SlotTables t;
                for (unsigned i = 0; i < ng; ++i) {
                    unsigned m, nq;
                    scanf("%u %u", &m, &nq);
                    std::vector<uint32_t> q(nq + 1);
                    for (unsigned j = 0; j < nq; ++j) scanf("%u", &q[j]);
                    t.add(base, m, q.data(), nq);
                    base += m;
                }
                printf("T %zu %u %zu %zu %zu\n", t.segs.size(), t.size(), t.slot_q.size(), t.slot_len.size(), t.slot_base.size());
                for (const SegGroup& g : t.segs) printf("g %u %u %u %u\n", g.list_base, g.m, g.slot0, g.nq);
                for (uint32_t i = 0; i < t.size(); ++i) printf("s %u %u %u\n", t.slot_q[i], t.slot_len[i], t.slot_base[i]);
                gs = t.segs;
            } else {
                for (unsigned i = 0; i < ng; ++i) {
                    unsigned m, nq;
                    scanf("%u %u", &m, &nq);
                    gs[i] = SegGroup{base, m, slot, nq};
                    slot += nq; base += m;
                }
            }
            const SegPlan p = limit ? plan_segments(gs, limit) : plan_segments(gs);
            printf("P %zu %zu\n", p.entries.size(), p.chunks.size());
            for (const SegChunk& c : p.chunks) {
                printf("C %u %u %u %u %u %u\n", c.e0, c.e1, c.slot0, c.n_slots, c.n_blocks, c.max_m);
                for (uint32_t b = 0; b < c.n_blocks; ++b) {
                    const SegBlock w = seg_lookup(p.entries.data() + c.e0, c.e1 - c.e0, b);
                    const SegEntry& e = p.entries[c.e0 + w.entry];
                    printf("B %u %u %u %u %u %u %u %u\n", c.e0 + w.entry, w.sub, w.tile, e.list_base, e.m, e.slot0, e.nq, e.nqc);
                }
            }
        }
    }
    return 0;
}
'''

LABEL_CASES = [
    [5],
    [7, 7, 7, 7],
    [3, 1, 3, 2, 1, 3, 0xFFFFFFFF, 0, 3],
    list(range(40, 0, -1)),                      # nq distinct labels, descending
    [9] * 8 + [4] * 9 + [9],
]

M_SET = [0, 1, 63, 64, 65]
NQ_SET = [1, 8, 9]


def seg_cases():
    cs = []
    for m, nq in itertools.product(M_SET, NQ_SET):
        cs.append(([(m, nq)], 0))
    cs.append(([(m, nq) for m, nq in itertools.product(M_SET, NQ_SET)], 0))           # all of them in one batch
    cs.append(([(m, nq) for m, nq in itertools.product(M_SET + [200, 8193], NQ_SET + [2, 3, 4, 5, 17])], 0))
    cs.append(([(65, 9), (0, 8), (130, 30), (1, 1), (64, 8)], 64 * 4 * 16))            # a limit of 16 slots of 64 columns
    cs.append(([(1000, 40), (10, 3)], 1024 * 4 * 8))                                   # one group cut into pieces of 8
    return cs


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("label_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


@pytest.mark.parametrize("labels", LABEL_CASES, ids=lambda l: f"nq{len(l)}")
def test_label_groups(run, labels):
    out = run(f"G {len(labels)} " + " ".join(str(x) for x in labels) + "\n")
    G = int(out[0].split()[1])
    got = [[int(x) for x in line.split()[1:]] for line in out[1:1 + G]]
    want = sorted(set(labels))
    assert [g[0] for g in got] == want
    for g in got:
        assert g[1:] == [i for i, l in enumerate(labels) if l == g[0]]      # every query of the label, ascending


def check_coverage(out, groups, limit):
    """`out`: the driver's lines from "P ..." on, for `groups` = [(m, nq)] laid out group after group."""
    n_entries, n_chunks = (int(x) for x in out[0].split()[1:])
    limit_bytes = limit or (1 << 30)
    slot0, base = [], []
    s = b = 0
    for m, nq in groups:
        slot0.append(s); base.append(b)
        s += nq; b += m
    total_slots = s
    owner = {}                                                   # slot -> (list_base, m)
    for (m, nq), s0, b0 in zip(groups, slot0, base):
        for j in range(nq):
            owner[s0 + j] = (b0, m)
    seen = {}
    next_slot = 0
    i = 1
    entries_seen = set()
    for _ in range(n_chunks):
        e0, e1, c_slot0, n_slots, n_blocks, max_m = (int(x) for x in out[i].split()[1:])
        i += 1
        assert c_slot0 == next_slot and n_slots > 0                # the chunks partition the slots, in order
        next_slot += n_slots
        cols = max(1, -(-max_m // 64) * 64) if max_m else 64
        assert n_slots * cols * 4 <= limit_bytes or n_slots <= 8
        prev = None
        for blk in range(n_blocks):
            e, sub, tile, lb, m, es0, enq, nqc = (int(x) for x in out[i].split()[1:])
            i += 1
            assert e0 <= e < e1 and m > 0
            entries_seen.add(e)
            assert nqc in (1, 2, 4, 8) and nqc == (8 if enq >= 5 else 4 if enq >= 3 else enq)
            assert tile * 64 < m
            first = es0 + sub * nqc
            n_own = min(nqc, enq - sub * nqc)
            assert n_own >= 1
            for sl in range(first, first + n_own):
                assert c_slot0 <= sl < c_slot0 + n_slots           # the block writes inside its chunk's score block
                assert owner[sl] == (lb, m)                        # ... the rows of the slot's own group
                assert max_m >= m
                key = (sl, tile)
                assert key not in seen
                seen[key] = True
            if prev is not None and prev[0] == e and prev[2] == tile:
                assert sub == prev[1] + 1                          # the subgroups of one tile are neighbouring blocks
            prev = (e, sub, tile)
    assert next_slot == total_slots
    assert entries_seen == set(range(n_entries))
    want = {(sl, t) for sl, (lb, m) in owner.items() for t in range(-(-m // 64))}
    assert set(seen) == want


@pytest.mark.parametrize("case", range(len(seg_cases())))
def test_work_table_covers_every_query_tile_pair_once(run, case):
    groups, limit = seg_cases()[case]
    check_coverage(run(f"S {len(groups)} {limit} " + " ".join(f"{m} {nq}" for m, nq in groups) + "\n"), groups, limit)


# (m, the group's queries): nq = 1, m = 0, several groups in a row, queries neither sorted nor distinct across groups
SLOT_CASES = [
    [(5, [7])],
    [(0, [3, 1])],
    [(65, [4, 0, 9]), (0, [2]), (1, [8]), (130, list(range(30, 10, -1))), (0, [5, 6]), (64, [1, 1, 3])],
    [(m, list(range(100 * i, 100 * i + nq))) for i, (m, nq) in enumerate(itertools.product(M_SET + [200], NQ_SET + [2, 5, 17]))],
]


@pytest.mark.parametrize("limit", [0, 64 * 4 * 16])
@pytest.mark.parametrize("case", range(len(SLOT_CASES)))
def test_slot_tables(run, case, limit):
    groups = SLOT_CASES[case]
    out = run(f"T {len(groups)} {limit} " + " ".join(f"{m} {len(qs)} " + " ".join(map(str, qs)) for m, qs in groups) + "\n")
    n_slots = sum(len(qs) for _, qs in groups)
    assert [int(x) for x in out[0].split()[1:]] == [len(groups), n_slots, n_slots, n_slots, n_slots]
    segs = [tuple(int(x) for x in line.split()[1:]) for line in out[1:1 + len(groups)]]
    slots = [tuple(int(x) for x in line.split()[1:]) for line in out[1 + len(groups):1 + len(groups) + n_slots]]
    slot0 = base = 0
    for (m, qs), seg in zip(groups, segs):
        assert seg == (base, m, slot0, len(qs))                      # slot0: the running slot count
        mine = slots[slot0:slot0 + len(qs)]
        assert [s[0] for s in mine] == qs                            # its queries, in the order given
        assert all(s[1] == m and s[2] == base for s in mine)         # m and list_base, once per query
        slot0 += len(qs)
        base += m
    check_coverage(out[1 + len(groups) + n_slots:], [(m, len(qs)) for m, qs in groups], limit)
