"""The host decisions of a search (vrod_amd/csrc/search_plan.h), checked on the host: a small driver is compiled with
g++ against the real header and prints its decisions over grids of inputs; this file states the rules and compares.

What is tied together here: the route (AUTO thresholds, split eligibility, the graph-replay predicate), k' per path and
the margin multiplier's state machine, the stage plan against test_gpu_steal.stage_plan, the fast pass's error bound
against certificate_fixtures.mfma_eps, the band-pass gate, and the k' values the GPU tests pin.  A rule changed in the
header without its restatements (or the other way round) fails here, not only on a GPU run."""
import math
import os
import shutil
import subprocess

import pytest

import certificate_fixtures as F
from test_gpu_steal import stage_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")

AUTO, STREAM, MFMA, EXACT = 0, 1, 2, 3
F32, BF16 = 0, 1
COSINE, L2, IP = 0, 1, 2
CAP = 8192

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "search_plan.h"
using namespace vrod;

int main(int argc, char** argv) {
    const char* mode = argv[1];
    if (!strcmp(mode, "route")) {          // dtype split_enabled skinny forced N k nq -> path split graph
        const unsigned skinny[] = {0, 16, 32};
        const unsigned long long Ns[] = {0, 100000};
        const unsigned ks[] = {10, 3000};
        for (int dtype = 0; dtype < 2; ++dtype)
        for (int se = 0; se < 2; ++se)
        for (unsigned sk : skinny)
        for (int forced = 0; forced < 4; ++forced)
        for (unsigned long long N : Ns)
        for (unsigned k : ks)
        for (unsigned nq = 1; nq <= 300; ++nq) {
            const Route r = route(forced, dtype, se != 0, sk, N, nq, k);
            printf("%d %d %u %d %llu %u %u %d %d %d\n", dtype, se, sk, forced, N, k, nq, r.path, (int)r.split,
                   (int)graph_route(forced, nq));
        }
    } else if (!strcmp(mode, "plan")) {    // path split metric dim N nq k boost margin -> kp eps_mode eps_c nq_pad N
        const SearchPlan p = make_plan(atoi(argv[2]), atoi(argv[3]) != 0, score_form(atoi(argv[4])), (uint32_t)atoi(argv[5]),
                                       strtoull(argv[6], 0, 10), (uint32_t)atoi(argv[7]), (uint32_t)atoi(argv[8]),
                                       (uint32_t)atoi(argv[9]), (uint32_t)atoi(argv[10]));
        printf("%u %d %.9e %u %llu %d %d\n", p.kp, p.eps_mode, (double)p.eps_c, p.nq_pad, (unsigned long long)p.N, p.path, (int)p.split);
    } else if (!strcmp(mode, "stages")) {  // N kp max_sample_rows -> S j bounds...
        const StagePlan sp = plan_stages(strtoull(argv[2], 0, 10), (uint32_t)atoi(argv[3]), kSelectChunk, (uint32_t)atoi(argv[4]), 0, 0);
        printf("%u %u", sp.S, sp.j);
        for (uint64_t b : sp.bounds) printf(" %llu", (unsigned long long)b);
        printf("\n");
    } else if (!strcmp(mode, "bound")) {   // mode c qn2 xn2 -> eps_bound
        printf("%.9e\n", (double)eps_bound(atoi(argv[2]), (float)atof(argv[3]), (float)atof(argv[4]), (float)atof(argv[5])));
    } else if (!strcmp(mode, "boost")) {   // verdicts F / C (run with the current multiplier) or F:u / C:u -> boost after each
        KpBoost s;
        for (int i = 2; i < argc; ++i) {
            const uint32_t used = argv[i][1] == ':' ? (uint32_t)atoi(argv[i] + 2) : s.boost;
            kp_boost_step(s, used, argv[i][0] == 'F');
            printf("%u ", s.boost);
        }
        printf("\n");
    } else if (!strcmp(mode, "band")) {    // path split eps_mode dtype nf k N nq_pad -> eligible
        SearchPlan p;
        p.path = atoi(argv[2]); p.split = atoi(argv[3]) != 0; p.eps_mode = atoi(argv[4]);
        p.N = strtoull(argv[8], 0, 10); p.nq_pad = (uint32_t)atoi(argv[9]);
        printf("%d\n", (int)band_eligible(p, atoi(argv[5]), (uint32_t)atoi(argv[6]), (uint32_t)atoi(argv[7])));
    } else if (!strcmp(mode, "forms")) {
        printf("%d %d %d %d %d %d\n", score_form(VROD_METRIC_COSINE), score_form(VROD_METRIC_L2), score_form(VROD_METRIC_IP),
               prep_form(VROD_METRIC_COSINE), prep_form(VROD_METRIC_L2), prep_form(VROD_METRIC_IP));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    if CXX is None:
        pytest.skip("needs a host C++ compiler")
    d = tmp_path_factory.mktemp("search_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    r = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120, check=True).stdout
        return out.split("\n")[:-1]
    return run


def plan(drv, path, split, metric, dim, n, nq, k, boost=1, margin=0):
    kp, mode, c, nq_pad, N, p, s = drv("plan", path, int(split), metric, dim, n, nq, k, boost, margin)[0].split()
    return {"kp": int(kp), "eps_mode": int(mode), "eps_c": float(c), "nq_pad": int(nq_pad), "N": int(N), "path": int(p),
            "split": bool(int(s))}


# ------------------------------------------------------------------ route
def expected_route(dtype, split_enabled, skinny, forced, n, k, nq):
    """AUTO: bf16 rows and fp32 split batches that fit the skinny kernel go to the MFMA path above 4 queries, other split
    batches above 12, fp32 above 32.  The graph predicate is AUTO with <= 4 queries or STREAM forced: narrower than the
    route for fp32 batches of 5..32 queries (which stream, but are not replayed)."""
    can_split = split_enabled and dtype == F32 and n > 0 and k + max(32, k // 2) <= CAP // 2
    skinny_split = can_split and nq <= skinny
    path = forced
    if forced == AUTO:
        limit = 4 if dtype == BF16 or skinny_split else 12 if can_split else 32
        path = STREAM if nq <= limit else MFMA
    return path, can_split and path == MFMA, forced == STREAM or (forced == AUTO and nq <= 4)


def test_routing_table(drv):
    rows = drv("route")
    assert len(rows) == 2 * 2 * 3 * 4 * 2 * 2 * 300
    wider = 0
    for line in rows:
        dtype, se, sk, forced, n, k, nq, path, split, graph = map(int, line.split())
        assert (path, bool(split), bool(graph)) == expected_route(dtype, se, sk, forced, n, k, nq), line
        wider += graph == 0 and path == STREAM and forced == AUTO and dtype == F32 and 5 <= nq <= 8
    # fp32 batches of 5..8 queries take the stream path but are never replayed from a graph
    assert wider > 0


# ------------------------------------------------------------------ k' and the stage plan
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("n", [1_500_000, 1_300_000, 1_850_000])
@pytest.mark.parametrize("num_cus", [256, 80, 304])
def test_stage_plan_equals_test_gpu_steal(drv, metric, n, num_cus):
    nq, k = 1024, 10
    kp, S, bounds = stage_plan(n, nq, k, metric, num_cus)
    p = plan(drv, MFMA, False, {"cosine": COSINE, "l2": L2}[metric], 192, n, nq, k)
    assert p["kp"] == kp and p["nq_pad"] == 1024
    got = list(map(int, drv("stages", n, kp, max(1, num_cus // (nq // 256)) * 256)[0].split()))
    assert got[0] == S and got[1] == min(kp, S) and got[2:] == bounds


def test_stage_plan_invariants(drv):
    checked = 0
    for n in (8193, 10_000, 65_536, 100_000, 1_300_001, 10_000_000, (1 << 25) + 7):
        for k in (1, 10, 100, 1000, 4096):
            for metric in (COSINE, L2):
                for boost in (1, 8):
                    kp = plan(drv, MFMA, False, metric, 768, n, 1024, k, boost)["kp"]
                    assert k <= kp <= CAP // 2 or kp == CAP // 2, (n, k, kp)
                    for max_sample in (256, 64 * 256, 256 * 256):
                        S, j, *bounds = map(int, drv("stages", n, kp, max_sample)[0].split())
                        what = (n, k, kp, max_sample, S, j, bounds)
                        assert all(a < b for a, b in zip(bounds, bounds[1:])), what
                        assert all(b % 256 == 0 for b in bounds[:-1]), what
                        assert bounds[-1] == n, what
                        assert S <= n and (S % 256 == 0 or S == n), what
                        assert j <= kp, what
                        checked += 1
    assert checked > 100


def test_pinned_kprime(drv):
    # test_gpu_margin: k = 10 over 50 000 bf16 cosine rows with the multiplier at 1, 2, 4 -> 18, 26, 42; k = 4096 at x4
    assert [plan(drv, MFMA, False, COSINE, 64, 50_000, 16, 10, b)["kp"] for b in (1, 2, 4)] == [18, 26, 42]
    assert plan(drv, MFMA, False, COSINE, 64, 50_000, 6, 4096, 4)["kp"] == 4096
    assert plan(drv, MFMA, False, COSINE, 64, 50_000, 6, 4096, 8)["kp"] == 4096
    # test_gpu_margin: k = 100 starts at k + 12 and doubles to k + 24
    assert plan(drv, MFMA, False, COSINE, 3072, 100_000, 64, 100, 1)["kp"] == 112
    assert plan(drv, MFMA, False, COSINE, 3072, 100_000, 64, 100, 2)["kp"] == 124
    # test_gpu_split: the split pass keeps k + max(32, k / 2), the fp32 MFMA cosine pass k + 8
    assert plan(drv, MFMA, True, COSINE, 768, 100_000, 100, 10)["kp"] == 10 + 32
    assert plan(drv, MFMA, False, COSINE, 768, 100_000, 100, 10)["kp"] == 10 + 8
    for n, k in ((30, 10), (5000, 10), (5000, 100), (5000, 1000)):
        assert plan(drv, MFMA, True, L2, 768, n, 100, k)["kp"] == min(n, k + max(32, k // 2))
    # L2 keeps a margin of 16; IP takes the dot-form margin of 8; VROD_DEBUG_KP_MARGIN replaces the 8 only
    assert plan(drv, MFMA, False, L2, 768, 100_000, 100, 10)["kp"] == 26
    assert plan(drv, MFMA, False, IP, 768, 100_000, 100, 10)["kp"] == 18
    assert plan(drv, MFMA, False, COSINE, 768, 100_000, 100, 10, 1, 4)["kp"] == 14
    assert plan(drv, MFMA, False, L2, 768, 100_000, 100, 10, 1, 4)["kp"] == 26
    # stream and exact paths: k + max(16, k / 8), no multiplier, inside N and the select window
    for path in (STREAM, EXACT):
        for n, k, boost in ((100_000, 10, 4), (100_000, 1000, 1), (20, 10, 1), (100_000, 4096, 8)):
            assert plan(drv, path, False, COSINE, 768, n, 4, k, boost)["kp"] == min(n, CAP // 2, k + max(16, k // 8))
    # an empty corpus: no candidates
    assert plan(drv, MFMA, False, COSINE, 768, 0, 4, 10)["kp"] == 0
    # the query block the lists and thresholds are sized by
    assert plan(drv, MFMA, False, COSINE, 768, 100, 300, 10)["nq_pad"] == 512
    assert plan(drv, STREAM, False, COSINE, 768, 100, 3, 10)["nq_pad"] == 8


# ------------------------------------------------------------------ the fast pass's error bound
@pytest.mark.parametrize("dim", [64, 192, 768, 3072])
def test_mfma_bound_equals_certificate_fixtures(drv, dim):
    for metric, name in ((COSINE, "cosine"), (L2, "l2")):
        for split in (False, True):
            p = plan(drv, MFMA, split, metric, dim, 100_000, 256, 10)
            assert p["eps_mode"] == (0 if metric == COSINE else 2)
            for qn, xn in ((1.0, 1.0), (0.25, 3.0), (7.5, 0.01), (1e3, 1e-2)):
                want = F.mfma_eps(dim, name, split, qn, xn)
                got = float(drv("bound", p["eps_mode"], repr(p["eps_c"]), repr(qn * qn), repr(xn * xn))[0])
                assert math.isclose(got, want, rel_tol=2e-6), (dim, name, split, qn, xn, got, want)


@pytest.mark.parametrize("dim", [64, 768, 3072])
def test_stream_and_exact_bounds(drv, dim):
    u = 2.0 ** -24
    p = plan(drv, STREAM, False, COSINE, dim, 100_000, 4, 10)
    assert p["eps_mode"] == 0 and math.isclose(p["eps_c"], 4 * dim * u, rel_tol=1e-6)
    assert plan(drv, STREAM, False, IP, dim, 100_000, 4, 10)["eps_c"] == p["eps_c"]
    p = plan(drv, STREAM, False, L2, dim, 100_000, 4, 10)
    assert p["eps_mode"] == 1 and math.isclose(p["eps_c"], 4 * (dim + 2) * u, rel_tol=1e-6)
    # mode 1 is relative: the norms do not enter
    assert float(drv("bound", 1, repr(p["eps_c"]), 9.0, 4.0)[0]) == pytest.approx(p["eps_c"], rel=1e-7)
    # the exact path has no fast pass
    p = plan(drv, EXACT, False, L2, dim, 100_000, 4, 10)
    assert p["eps_mode"] == 0 and p["eps_c"] == 0.0


def test_score_forms(drv):
    # COSINE and IP score in the dot form, L2 in its own; only COSINE normalises the rows
    assert drv("forms")[0].split() == ["0", "1", "0", "0", "1", "1"]


# ------------------------------------------------------------------ the margin multiplier
def boosts(drv, *verdicts):
    return list(map(int, drv("boost", *verdicts)[0].split()))


def test_kp_boost_doubles_on_failures_and_halves_after_64_clean(drv):
    # test_gpu_margin: a search with failures doubles the multiplier (k' = k + 12 -> k + 24), and again (x4: 42 at k = 10)
    assert boosts(drv, "F", "F") == [2, 4]
    assert boosts(drv, "F", "C", "C") == [2, 2, 2]
    b = boosts(drv, "F", *["C"] * 64)
    assert b[:-1] == [2] * 64 and b[-1] == 1           # the 64th clean search halves it
    b = boosts(drv, "F", "F", *["C"] * 128)
    assert b[64] == 4 and b[65] == 2 and b[128] == 2 and b[129] == 1
    assert boosts(drv, "F", *["C"] * 30, "F", *["C"] * 63)[-1] == 4   # a failure restarts the clean count
    # a verdict counts only for the multiplier its search ran with (two searches in flight)
    assert boosts(drv, "F", "F:1") == [2, 2]
    assert boosts(drv, "F", *["C:1"] * 64) == [2] * 65


def test_kp_boost_resets_at_8_and_holds_256(drv):
    b = boosts(drv, "F", "F", "F", "F")
    assert b == [2, 4, 8, 1]                           # failures at x8: the margin is not what they lack
    b = boosts(drv, *["F"] * (4 + 256))
    assert b[4:4 + 255] == [1] * 255 and b[4 + 255] == 2   # 255 searches held at 1, the 256th doubles again
    b = boosts(drv, "F", "F", "F", "F", *["C"] * 300)
    assert set(b[4:]) == {1}


# ------------------------------------------------------------------ band-pass gate
def test_band_gate(drv):
    def band(path=MFMA, split=0, eps_mode=0, dtype=BF16, nf=2, k=10, n=100_000, nq_pad=256):
        return drv("band", path, split, eps_mode, dtype, nf, k, n, nq_pad)[0] == "1"

    assert band() and not band(nf=1)                       # bf16 rows: from 2 failed queries on
    assert not band(dtype=F32, nf=47) and band(dtype=F32, nf=48)   # fp32 MFMA pass: from 48
    assert band(dtype=F32, split=1, nf=2)                  # the split pass scans bf16 planes: from 2
    assert band(eps_mode=2)
    assert not band(path=STREAM) and not band(path=EXACT)
    assert not band(eps_mode=1)                            # a relative bound has no band
    assert not band(k=10, n=9) and band(k=10, n=10)
    assert not band(nq_pad=0)
