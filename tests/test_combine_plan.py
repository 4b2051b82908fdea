"""The host-side plan of vrod_search_combined (vrod_amd/csrc/combine_plan.h), checked on the host: a small driver is
compiled with g++ against the real header.

  - the constants restate the ABI and the Python package;
  - k1 = k + the batch's largest excluded count, terms counted under the flag;
  - every limit at its edge: 256 / 257 terms, 1024 / 1025 excluded entries (with and without the terms in them),
    k + excluded = VROD_MAX_K and one more, k = 0, k past VROD_MAX_K, unknown flag bits;
  - lims arrays that do not start at 0 or that decrease, a query without an operand;
  - the lanes that own a query in the combine launch, on both sides of the switch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
HDR = open(os.path.join(ROOT, "include", "vrod.h")).read()
MAX_K = int(re.search(r"#define VROD_MAX_K (\d+)u", HDR).group(1))
MAX_TERMS = int(re.search(r"#define VROD_MAX_COMBINE_TERMS (\d+)u", HDR).group(1))
MAX_EXCLUDE = int(re.search(r"#define VROD_MAX_EXCLUDE (\d+)u", HDR).group(1))

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "combine_plan.h"
using namespace vrod;

static std::vector<uint32_t> read_lims(unsigned n) {
    std::vector<uint32_t> v(n);
    for (unsigned i = 0; i < n; ++i) scanf("%u", &v[i]);
    return v;
}

int main() {
    char what;
    printf("M %u %u %u %u\n", kCombineMaxK, kCombineMaxTerms, kCombineMaxExclude, kCombineExcludeTerms);
    while (scanf(" %c", &what) == 1) {
        if (what == 'A') {          // the arguments alone
            unsigned k, flags;
            scanf("%u %u", &k, &flags);
            printf("A %d\n", combine_check_args(k, flags));
        } else if (what == 'L') {   // lanes per query
            unsigned dim, eb;
            scanf("%u %u", &dim, &eb);
            printf("L %u\n", combine_lanes_per_query(dim, eb));
        } else {                    // a batch: nq has_vector k flags has_excl, term lims, [exclude lims]
            unsigned nq, k, flags; int hv, hx;
            scanf("%u %d %u %u %d", &nq, &hv, &k, &flags, &hx);
            std::vector<uint32_t> tl = read_lims(nq + 1), xl;
            if (hx) xl = read_lims(nq + 1);
            CombineCounts c;
            uint32_t bad = 0;
            const int rc = combine_check_batch(tl.data(), hx ? xl.data() : nullptr, nq, hv != 0, k, flags, &c, &bad);
            printf("B %d %u %u %u %u\n", rc, rc >= 5 && rc <= 7 ? bad : 0u, c.max_terms, c.max_excluded, rc ? 0u : combine_search_k(k, c.max_excluded));
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not CXX:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("combine_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def go(text):
        return subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return go


def batch(run, term_lims, excl_lims=None, has_vector=False, k=10, flags=0):
    nq = len(term_lims) - 1
    line = f"B {nq} {int(has_vector)} {k} {flags} {int(excl_lims is not None)} " + " ".join(map(str, term_lims))
    if excl_lims is not None:
        line += " " + " ".join(map(str, excl_lims))
    out = run(line + "\n")[1].split()
    assert out[0] == "B"
    return tuple(int(x) for x in out[1:])   # (rc, bad query, max terms, max excluded, k1)


def test_constants_follow_the_abi_and_the_package(run):
    import vrod_amd
    assert run("")[0].split() == ["M", str(MAX_K), str(MAX_TERMS), str(MAX_EXCLUDE), "1"]
    assert (vrod_amd.index.MAX_COMBINE_TERMS, vrod_amd.index.MAX_EXCLUDE, vrod_amd.index.COMBINED_EXCLUDE_TERMS) == (MAX_TERMS, MAX_EXCLUDE, 1)
    assert (MAX_TERMS, MAX_EXCLUDE) == (256, 1024)


def test_k1_is_k_plus_the_largest_excluded_count(run):
    # three queries: 2, 5, 1 terms; 0, 3, 7 excluded
    tl, xl = [0, 2, 7, 8], [0, 0, 3, 10]
    assert batch(run, tl) == (0, 0, 5, 0, 10)                               # nothing excluded: the search runs with k
    assert batch(run, tl, flags=1) == (0, 0, 5, 5, 15)                      # the terms alone
    assert batch(run, tl, xl) == (0, 0, 5, 7, 17)                           # the lists alone
    assert batch(run, tl, xl, flags=1) == (0, 0, 5, 8, 18)                  # per query 2, 8, 8: sums, then the maximum
    assert batch(run, tl, [0, 0, 0, 0], flags=0) == (0, 0, 5, 0, 10)        # an exclude list that is empty everywhere
    assert batch(run, [0, 0, 0], has_vector=True) == (0, 0, 0, 0, 10)       # vectors only


def test_limits_at_their_edges(run):
    assert batch(run, [0, MAX_TERMS])[0] == 0
    assert batch(run, [0, 1, 1 + MAX_TERMS + 1])[:2] == (6, 1)
    assert batch(run, [0, 1], [0, MAX_EXCLUDE], k=1)[0] == 0
    assert batch(run, [0, 1], [0, MAX_EXCLUDE + 1], k=1)[:2] == (7, 0)
    # under the flag the terms count: 1024 - 256 listed + 256 terms fits, one more listed id does not
    assert batch(run, [0, MAX_TERMS], [0, MAX_EXCLUDE - MAX_TERMS], k=1, flags=1)[:4] == (0, 0, MAX_TERMS, MAX_EXCLUDE)
    assert batch(run, [0, MAX_TERMS], [0, MAX_EXCLUDE - MAX_TERMS + 1], k=1, flags=1)[:2] == (7, 0)
    assert batch(run, [0, MAX_TERMS], [0, MAX_EXCLUDE - MAX_TERMS + 1], k=1, flags=0)[0] == 0
    # k + excluded against VROD_MAX_K
    assert batch(run, [0, 1], [0, 300], k=MAX_K - 300) == (0, 0, 1, 300, MAX_K)
    assert batch(run, [0, 1], [0, 300], k=MAX_K - 299)[0] == 8
    assert batch(run, [0, 1, 2], [0, 0, 1], k=MAX_K)[0] == 8                # one excluded id anywhere in the batch
    assert batch(run, [0, 1, 2], [0, 0, 0], k=MAX_K)[0] == 0
    assert batch(run, [0, 1], k=MAX_K, flags=1)[0] == 8                     # ... the term itself under the flag
    # lims entries near 2^32 do not wrap the excluded count into range
    assert batch(run, [0, 0xFFFFFFFF], [0, 0xFFFFFFFF], flags=1)[0] == 6
    out = run("".join(f"A {k} {f}\n" for k, f in [(1, 0), (MAX_K, 1), (0, 0), (MAX_K + 1, 0), (5, 2), (5, 0x80000001), (0, 2)]))[1:]
    assert [int(l.split()[1]) for l in out] == [0, 0, 2, 2, 1, 1, 1]


def test_bad_lims_and_missing_operands(run):
    assert batch(run, [1, 2])[0] == 3
    assert batch(run, [0, 3, 2])[0] == 3
    assert batch(run, [0, 1, 2], [1, 1, 1])[0] == 4
    assert batch(run, [0, 1, 2], [0, 2, 1])[0] == 4
    assert batch(run, [0, 1, 1, 2])[:2] == (5, 1)                            # query 1 has no term and there is no vector
    assert batch(run, [0, 1, 1, 2], has_vector=True)[0] == 0


def test_lanes_per_query(run):
    # a wave while the stored row is at most 256 16-B units (1024 fp32, 2048 bf16 values), the work-group beyond
    cases = [(1, 4, 64), (1024, 4, 64), (1025, 4, 256), (4100, 4, 256), (2048, 2, 64), (2049, 2, 256), (1100, 2, 64), (1100, 4, 256)]
    out = run("".join(f"L {d} {e}\n" for d, e, _ in cases))[1:]
    assert [int(l.split()[1]) for l in out] == [w for _, _, w in cases]
