"""The host-side plan of a tagged search (vrod_amd/csrc/tag_plan.h), checked on the host: a small driver is compiled with
g++ against the real header.

  - tag_matches: the three clauses of the predicate, on 64-bit values;
  - tag_groups: identical (any, all, none) triples merged, the groups ordered by the triple, every query of a satisfiable
    predicate in exactly one group and ascending within it; queries of unsatisfiable predicates (all & none != 0) in no
    group, counted apart;
  - plan_tag_passes with a small byte cap: every narrow group in exactly one pass, at its own offset of the pass's list
    buffer, lists packed without gaps; no pass over the cap (a single group larger than the cap aside: served alone) or
    over the groups-per-pass limit; wide groups get kNoSegment; a run of wide groups makes no pass."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
NO_SEGMENT = 0xFFFFFFFF

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "tag_plan.h"
using namespace vrod;

int main() {
    static_assert(sizeof(TagPred) == 24, "TagPred");
    static_assert(kTagGroupsPerPass * kTagLdsPerGroup <= 64 * 1024, "the pass's table fits the LDS of a plain launch");
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            printf("K %u\n", kTagGroupsPerPass);
        } else if (what == 'M') {
            unsigned long long t, a, b, c;
            scanf("%llx %llx %llx %llx", &t, &a, &b, &c);
            printf("M %d\n", (int)tag_matches(t, a, b, c));
        } else if (what == 'G') {
            unsigned nq;
            scanf("%u", &nq);
            std::vector<TagPred> p(nq + 1);
            for (unsigned i = 0; i < nq; ++i) {
                unsigned long long a, b, c;
                scanf("%llx %llx %llx", &a, &b, &c);
                p[i] = TagPred{a, b, c};
            }
            const TagGroups g = tag_groups(p.data(), nq);
            printf("G %u %u\n", g.size(), g.n_unsatisfiable());
            for (uint32_t i = 0; i < g.size(); ++i) {
                printf("L %llx %llx %llx", (unsigned long long)g.preds[i].any, (unsigned long long)g.preds[i].all, (unsigned long long)g.preds[i].none);
                for (uint32_t j = g.q_off[i]; j < g.q_off[i + 1]; ++j) printf(" %u", g.q_order[j]);
                printf("\n");
            }
            printf("U");
            for (uint32_t j = g.q_off[g.size()]; j < nq; ++j) printf(" %u", g.q_order[j]);
            printf("\n");
        } else {
            unsigned ng, max_groups;
            unsigned long long cap;
            scanf("%u %llu %u", &ng, &cap, &max_groups);
            std::vector<uint32_t> m(ng);
            std::vector<uint8_t> narrow(ng);
            for (unsigned i = 0; i < ng; ++i) {
                unsigned a, b;
                scanf("%u %u", &a, &b);
                m[i] = a; narrow[i] = (uint8_t)b;
            }
            const std::vector<TagPass> ps = !cap ? plan_tag_passes(m, narrow) : !max_groups ? plan_tag_passes(m, narrow, cap)
                                                                                            : plan_tag_passes(m, narrow, cap, max_groups);
            printf("P %zu\n", ps.size());
            for (const TagPass& p : ps) {
                printf("T %u %u %u %llu", p.g0, p.g1, p.n_lists, (unsigned long long)p.list_n);
                for (uint32_t o : p.seg_off) printf(" %u", o);
                printf("\n");
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
    d = tmp_path_factory.mktemp("tag_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def matches(t, any_, all_, none):
    return (any_ == 0 or (t & any_) != 0) and (t & all_) == all_ and (t & none) == 0


def test_constant_matches_the_source(run):
    text = open(os.path.join(CSRC, "tag_plan.h")).read()
    import re
    k = int(re.search(r"constexpr uint32_t kTagGroupsPerPass = (\d+);", text).group(1))
    assert run("K\n") == [f"K {k}"] and k >= 64


def test_tag_matches(run):
    B0, B31, B32, B63 = 1, 1 << 31, 1 << 32, 1 << 63
    cases = []
    for t in (0, B0, B63, B0 | B63, B31, B32, B31 | B32, (1 << 64) - 1):
        for p in ((0, 0, 0), (B63, 0, 0), (B0, 0, 0), (B0 | B63, 0, 0), (0, B0 | B63, 0), (0, B32, 0), (0, 0, B63), (0, 0, B32),
                  (B31, 0, B32), (B0, B63, B31), (0, B63, B63), ((1 << 64) - 1, 0, 0)):
            cases.append((t, *p))
    out = run("".join("M %x %x %x %x\n" % c for c in cases))
    assert [int(l.split()[1]) for l in out] == [int(matches(*c)) for c in cases]
    assert any(matches(*c) for c in cases) and not all(matches(*c) for c in cases)


B63 = 1 << 63
PRED_CASES = [
    [(1, 0, 0)],
    [(5, 1, 2)] * 4,
    [(B63, 0, 0), (1, 0, 0), (B63, 0, 0), (0, 0, 0), (1, 2, 0), (1, 0, 2), (1, 0, 0), (0, 3, 1), (0, 0, 0), (0, B63, B63), (1, 0, 0)],
    [(0, 1, 1), (0, B63 | 1, B63)],                                                   # nothing but unsatisfiable ones
    [(i % 7, i % 3, 0) for i in range(40, 0, -1)],
    [(1, 2, 4), (1, 4, 2), (2, 1, 4), (1, 2, 4), (0, 6, 2), (1, 2, 5)],
]


@pytest.mark.parametrize("preds", PRED_CASES, ids=lambda p: f"nq{len(p)}")
def test_tag_groups(run, preds):
    out = run(f"G {len(preds)} " + " ".join("%x %x %x" % p for p in preds) + "\n")
    G, n_unsat = (int(x) for x in out[0].split()[1:])
    got = [line.split()[1:] for line in out[1:1 + G]]
    sat = sorted({p for p in preds if not p[1] & p[2]})
    assert [tuple(int(x, 16) for x in g[:3]) for g in got] == sat                   # merged, ordered by the triple
    for g in got:
        p = tuple(int(x, 16) for x in g[:3])
        assert [int(x) for x in g[3:]] == [i for i, x in enumerate(preds) if x == p]  # its queries, ascending
    unsat = [i for i, p in enumerate(preds) if p[1] & p[2]]
    assert n_unsat == len(unsat) and [int(x) for x in out[1 + G].split()[1:]] == unsat


def pass_cases():
    rng = np.random.default_rng(3)
    cs = [
        ([(10, 1)], 64, 0),
        ([(0, 1)], 64, 0),                                                           # an empty narrow group still gets a list
        ([(10, 0)], 64, 0),
        ([(1000, 0), (2000, 0)], 64, 0),                                              # wide groups only: no pass
        ([(8, 1), (8, 1), (1, 1)], 64, 0),                                            # 16 entries fill the cap exactly
        ([(5, 1), (100, 1), (5, 1)], 64, 0),                                          # a group larger than the cap
        ([(5, 1), (9000, 0), (5, 1), (7, 1), (9000, 0), (3, 1)], 64, 0),
        ([(1, 1)] * 11, 1 << 20, 4),                                                 # the groups-per-pass limit alone
        ([(3, 1), (0, 1), (70, 0)] * 9, 40, 5),                                       # both limits
        ([(int(m), int(n)) for m, n in zip(rng.integers(0, 40, 300), rng.random(300) < 0.8)], 256, 16),
        ([(int(m), 1) for m in rng.integers(0, 100, 50)], 0, 0),                     # the defaults: one pass
    ]
    return cs


@pytest.mark.parametrize("case", range(len(pass_cases())))
def test_scatter_passes(run, case):
    groups, cap, max_groups = pass_cases()[case]
    out = run(f"P {len(groups)} {cap} {max_groups} " + " ".join(f"{m} {n}" for m, n in groups) + "\n")
    k = int(run("K\n")[0].split()[1])
    cap_bytes, limit = cap or (1 << 30), max_groups or k
    n_pass = int(out[0].split()[1])
    seen = {}
    prev_end = 0
    for line in out[1:1 + n_pass]:
        f = [int(x) for x in line.split()[1:]]
        g0, g1, n_lists, list_n, seg_off = f[0], f[1], f[2], f[3], f[4:]
        assert prev_end <= g0 < g1 <= len(groups) and len(seg_off) == g1 - g0   # consecutive groups, passes in order
        prev_end = g1
        assert g1 - g0 <= limit
        at = 0
        for g, off in zip(range(g0, g1), seg_off):
            m, narrow = groups[g]
            if not narrow:
                assert off == NO_SEGMENT                                             # a wide group gets no list
                continue
            assert off == at and g not in seen                                       # packed, in group order
            seen[g] = True
            at += m
        assert at == list_n and n_lists == sum(1 for g in range(g0, g1) if groups[g][1]) and n_lists > 0
        assert list_n * 4 <= cap_bytes or n_lists == 1                               # over the cap only alone
    assert sorted(seen) == [g for g, (m, narrow) in enumerate(groups) if narrow]     # every narrow group exactly once
    if case == len(pass_cases()) - 1:
        assert n_pass == 1
