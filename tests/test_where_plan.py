"""The host-side plan of a search with a tags + value-interval predicate (vrod_amd/csrc/where_plan.h), checked on the
host: a small driver is compiled with g++ against the real header, as test_tag_plan.py compiles tag_plan.h.

  - the sizes: WherePred is 40 bytes, 1024 groups of 44 bytes fit the 64 KiB LDS of a plain launch;
  - where_matches against its Python restatement (where_model.where_matches) on random inputs that sit on and around
    the sign boundary and the interval's ends;
  - where_unsatisfiable: lo > hi, or all & none != 0;
  - where_groups: identical predicates merged, the groups ordered by (any, all, none, lo, hi) with the ends signed,
    every query of a satisfiable predicate in exactly one group and ascending within it (q_off / q_order), the queries
    of unsatisfiable predicates last, in no group;
  - plan_tag_passes and kNoSegment reused as they are, with the groups-per-pass limit of this search."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from where_model import FULL, I64_MAX, I64_MIN, unsatisfiable, where_matches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
NO_SEGMENT = 0xFFFFFFFF

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "where_plan.h"
using namespace vrod;

int main() {
    static_assert(sizeof(WherePred) == 40, "WherePred");
    static_assert(kWhereGroupsPerPass == 1024 && kWhereLdsPerGroup == 44, "1024 predicates of 40 + 4 bytes per pass");
    static_assert(kWhereGroupsPerPass * kWhereLdsPerGroup <= 64 * 1024, "the pass's table fits the LDS of a plain launch");
    static_assert(kNoSegment == 0xFFFFFFFFu, "label_plan.h's marker, as it is");
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'K') {
            printf("K %u %u %zu\n", kWhereGroupsPerPass, kWhereLdsPerGroup, sizeof(WherePred));
        } else if (what == 'M') {
            unsigned long long t, a, b, c;
            long long v, lo, hi;
            scanf("%llx %lld %llx %llx %llx %lld %lld", &t, &v, &a, &b, &c, &lo, &hi);
            printf("M %d %d\n", (int)where_matches(t, v, a, b, c, lo, hi), (int)where_unsatisfiable(WherePred{a, b, c, lo, hi}));
        } else if (what == 'G') {
            unsigned nq;
            scanf("%u", &nq);
            std::vector<WherePred> p(nq + 1);
            for (unsigned i = 0; i < nq; ++i) {
                unsigned long long a, b, c;
                long long lo, hi;
                scanf("%llx %llx %llx %lld %lld", &a, &b, &c, &lo, &hi);
                p[i] = WherePred{a, b, c, lo, hi};
            }
            const WhereGroups g = where_groups(p.data(), nq);
            printf("G %u %u\n", g.size(), g.n_unsatisfiable());
            for (uint32_t i = 0; i < g.size(); ++i) {
                printf("L %llx %llx %llx %lld %lld :", (unsigned long long)g.preds[i].any, (unsigned long long)g.preds[i].all,
                       (unsigned long long)g.preds[i].none, (long long)g.preds[i].lo, (long long)g.preds[i].hi);
                for (uint32_t j = g.q_off[i]; j < g.q_off[i + 1]; ++j) printf(" %u", g.q_order[j]);
                printf("\n");
            }
            printf("U");
            for (uint32_t j = g.q_off[g.size()]; j < nq; ++j) printf(" %u", g.q_order[j]);
            printf("\n");
        } else {
            unsigned ng;
            scanf("%u", &ng);
            std::vector<uint32_t> m(ng, 1);
            std::vector<uint8_t> narrow(ng, 1);
            if (ng) narrow[ng / 2] = 0;
            const std::vector<TagPass> ps = plan_tag_passes(m, narrow, 1ull << 30, kWhereGroupsPerPass);
            printf("P %zu\n", ps.size());
            for (const TagPass& p : ps) printf("T %u %u %u %llu %u\n", p.g0, p.g1, p.n_lists, (unsigned long long)p.list_n, p.seg_off[ng / 2 >= p.g0 && ng / 2 < p.g1 ? ng / 2 - p.g0 : 0]);
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("where_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def test_sizes_match_the_source_and_the_lds(run):
    text = open(os.path.join(CSRC, "where_plan.h")).read()
    k = int(re.search(r"constexpr uint32_t kWhereGroupsPerPass = (\d+);", text).group(1))
    per = int(re.search(r"constexpr uint32_t kWhereLdsPerGroup = (\d+);", text).group(1))
    assert run("K\n") == [f"K {k} {per} 40"]
    assert k == 1024 and per == 40 + 4 and k * per == 44 * 1024 <= 64 * 1024
    assert "hip/" not in text and "__global__" not in text                       # host arithmetic only


def test_tag_plan_names_are_kept(run):
    text = open(os.path.join(CSRC, "tag_plan.h")).read()
    for name in ("struct TagPred", "tag_matches", "tag_unsatisfiable", "kTagGroupsPerPass", "kTagLdsPerGroup", "TagGroups", "tag_groups",
                 "struct TagPass", "plan_tag_passes"):
        assert name in text, name


EDGE = [I64_MIN, I64_MIN + 1, -(1 << 32) - 1, -(1 << 32), -(1 << 31), -2, -1, 0, 1, 2, (1 << 31) - 1, 1 << 31, 1 << 32, I64_MAX - 1, I64_MAX]


def test_where_matches_and_unsatisfiable(run):
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(3000):
        v, lo, hi = (int(x) for x in rng.choice(EDGE, 3))
        if rng.random() < 0.3:
            v = int(rng.integers(I64_MIN, I64_MAX, endpoint=True))
        t = int(rng.integers(0, 16)) | (int(rng.integers(0, 2)) << 63)
        a, b, c = (int(rng.integers(0, 16)) * int(rng.random() < 0.5) | (int(rng.random() < 0.2) << 63) for _ in range(3))
        cases.append((t, v, a, b, c, lo, hi))
    for v in EDGE:                                                               # both ends include a stored value
        cases += [(0, v, 0, 0, 0, v, v), (0, v, 0, 0, 0, I64_MIN, v), (0, v, 0, 0, 0, v, I64_MAX), (0, v, 0, 0, 0, *FULL)]
    cases += [(0, -3, 0, 0, 0, -5, 5), (0, -3, 0, 0, 0, 0, I64_MAX), (0, 3, 0, 0, 0, I64_MIN, -1)]   # the sign decides
    out = run("".join("M %x %d %x %x %x %d %d\n" % c for c in cases))
    got = [tuple(int(x) for x in line.split()[1:]) for line in out]
    want = [(int(where_matches(np.array([c[0]], np.uint64), np.array([c[1]], np.int64), c[2:])[0]), int(unsatisfiable(c[2:]))) for c in cases]
    assert got == want
    hits = [g[0] for g in got]
    assert 0.05 < sum(hits) / len(hits) < 0.95 and any(g[1] for g in got)
    assert all(not h for h, u in got if u)                                        # an unsatisfiable predicate matches no input


B63 = 1 << 63
PRED_CASES = [
    [(1, 0, 0, 0, 0)],
    [(5, 1, 2, -3, 3)] * 4,
    [(0, 0, 0, -1, 1), (0, 0, 0, 1, -1), (0, 0, 0, -1, 1), (B63, 0, 0, *FULL), (0, 0, 0, -2, 1), (0, 0, 0, -1, 2), (0, 1, 1, 0, 0),
     (0, 0, 0, I64_MIN, 1), (0, 0, 0, -1, I64_MAX), (1, 0, 0, -1, 1), (0, 0, 0, 0, 0), (0, 0, 0, *FULL), (B63, 0, 0, *FULL)],
    [(0, 1, 1, *FULL), (0, 0, 0, 5, 4), (0, B63 | 1, B63, 9, 8)],               # nothing but unsatisfiable ones
    [(i % 3, 0, 0, -(i % 5), i % 4) for i in range(60, 0, -1)],
    [(0, 0, 0, lo, hi) for lo in (1, -1, I64_MIN, 0) for hi in (I64_MAX, -1, 0, 1)],   # the order of the ends is signed
]


@pytest.mark.parametrize("preds", PRED_CASES, ids=lambda p: f"nq{len(p)}")
def test_where_groups(run, preds):
    out = run(f"G {len(preds)} " + " ".join("%x %x %x %d %d" % p for p in preds) + "\n")
    G, n_unsat = (int(x) for x in out[0].split()[1:])

    def pred_of(line):
        f = line.split()
        return tuple(int(x, 16) for x in f[1:4]) + (int(f[4]), int(f[5]))
    got = [(pred_of(line), [int(x) for x in line.split(":")[1].split()]) for line in out[1:1 + G]]
    sat = sorted({p for p in preds if not unsatisfiable(p)})                     # tuples of ints: the ends compare signed
    assert [g[0] for g in got] == sat                                            # merged, ordered by (any, all, none, lo, hi)
    for p, qs in got:
        assert qs == [i for i, x in enumerate(preds) if x == p]                  # its queries, ascending
    unsat = [i for i, p in enumerate(preds) if unsatisfiable(p)]
    assert n_unsat == len(unsat) and [int(x) for x in out[1 + G].split()[1:]] == unsat


@pytest.mark.parametrize("ng", [1, 1024, 1025, 2500])
def test_passes_use_this_search_s_limit(run, ng):
    """plan_tag_passes as it is, cut at kWhereGroupsPerPass: groups of one row each, the middle one wide."""
    out = run(f"P {ng}\n")
    n_pass = int(out[0].split()[1])
    passes = [[int(x) for x in line.split()[1:]] for line in out[1:1 + n_pass]]
    if ng == 1:
        assert n_pass == 0                                                       # the only group is wide: no pass
        return
    assert n_pass == -(-ng // 1024)
    at = 0
    for g0, g1, n_lists, list_n, off in passes:
        assert g0 == at and g1 - g0 <= 1024 and n_lists == list_n
        if g0 <= ng // 2 < g1:
            assert off == NO_SEGMENT and n_lists == g1 - g0 - 1
        else:
            assert n_lists == g1 - g0
        at = g1
    assert at == ng
