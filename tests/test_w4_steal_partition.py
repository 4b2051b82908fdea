"""The partition of a strip's tail into claimable chunks (work stealing of the 4-wave scan, vrod_amd/csrc/w4_steal.h),
checked on the host: a small driver is compiled with g++ against the real header for every A/B setting of
VROD_W4_STEAL_CHUNK x VROD_W4_STEAL_DIV and walks every strip length up to 200 000 tiles.

What the kernel's claim protocol needs (kernels_mfma_w4.hip, at the claim): the chunks of a strip tile its tail
[e - tail, e) exactly -- disjoint, ascending, no gap, so every tile is scanned once whoever claims it -- every chunk is
at least 2 tiles long (a 1-tile range would be claimed behind in the same advance that reads it), the chunks of a strip
fit one 32-bit word of claim bits, and short strips keep no tail.  (The arithmetic before w4_steal.h clipped the last
chunk: a tail of 3 became [2], [1].)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vrod_amd", "csrc")

DRIVER = r'''
#include <cstdio>
#include "w4_steal.h"
using namespace vrod;
int main() {
    const uint32_t base = 1000003u;    // a strip does not start at tile 0
    uint32_t odd_tails = 0;
    for (uint32_t n = 0; n <= 200000u; ++n) {
        const uint32_t b = base, e = base + n;
        const uint32_t tail = w4_tail_tiles(n), cpt = w4_tail_chunks(n);
        if (n < 48u && tail != 0u) { printf("FAIL n=%u: tail %u below 48 tiles\n", n, tail); return 1; }
        if (tail > n) { printf("FAIL n=%u: tail %u longer than the strip\n", n, tail); return 1; }
        if (cpt > 32u) { printf("FAIL n=%u: %u chunks, more than one claim word\n", n, cpt); return 1; }
        if ((tail == 0u) != (cpt == 0u)) { printf("FAIL n=%u: tail %u in %u chunks\n", n, tail, cpt); return 1; }
        odd_tails += tail & 1u;
        uint32_t at = e - tail;          // the chunks must tile [e - tail, e): ascending, disjoint, no gap
        for (uint32_t j = 0; j < cpt; ++j) {
            uint32_t cb = 0, ce = 0;
            w4_chunk_range(b, e, j, cb, ce);
            if (cb != at) { printf("FAIL n=%u: chunk %u starts at %u, expected %u\n", n, j, cb - b, at - b); return 1; }
            if (ce < cb + 2u) { printf("FAIL n=%u tail=%u: chunk %u is [%u, %u), shorter than 2 tiles\n", n, tail, j, cb - b, ce - b); return 1; }
            at = ce;
        }
        if (at != e) { printf("FAIL n=%u tail=%u: chunks end at %u, not at the strip's end %u\n", n, tail, at - b, n); return 1; }
    }
    printf("OK odd_tails=%u\n", odd_tails);
    return 0;
}
'''

CXX = shutil.which("g++") or shutil.which("c++")


def _compile(tmp_path, chunk, div):
    src = tmp_path / "w4_steal_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / f"driver_{chunk}_{div}"
    r = subprocess.run([CXX, "-std=c++17", "-O2", "-Wall", f"-DVROD_W4_STEAL_CHUNK={chunk}", f"-DVROD_W4_STEAL_DIV={div}",
                        "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True, timeout=120)
    return r, exe


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("div", [8, 16, 32])
@pytest.mark.parametrize("chunk", [2, 3, 4])
def test_tail_chunks_tile_the_tail_and_are_never_one_tile(tmp_path, chunk, div):
    r, exe = _compile(tmp_path, chunk, div)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout[-2000:]
    # odd tails occur in every setting (e.g. 3 at 48..63 tiles with the default 1/16): the folding rule is exercised
    assert int(out.stdout.split("odd_tails=")[1]) > 0, out.stdout


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("div", [8, 16, 32])
def test_one_tile_chunks_do_not_build(tmp_path, div):
    """VROD_W4_STEAL_CHUNK=1 would hand out 1-tile ranges: the header refuses it at compile time."""
    r, _ = _compile(tmp_path, 1, div)
    assert r.returncode != 0
    assert "1-tile" in r.stderr or "one tile" in r.stderr, r.stderr[-2000:]


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_default_tails_of_the_multi_gpu_shard_sizes_are_odd(tmp_path):
    """The strip lengths of the last filtered stage at the shard sizes of the multi-GPU plan (batch 1024, 64 strips):
    1.25M rows -> 51-52 tiles, 2.5M -> 127-128, 5M -> 180-181, and the odd-tail GPU tests' 1.3M -> 54-55, 1.85M -> 87-88.
    Their tails under the default 1/16 and what the partition makes of them."""
    drv = tmp_path / "tails.cpp"
    drv.write_text(r'''
#include <cstdio>
#include "w4_steal.h"
using namespace vrod;
int main() {
    const unsigned ns[] = {51, 52, 54, 55, 87, 88, 127, 128, 180, 181};
    for (unsigned n : ns) {
        printf("%u %u", n, w4_tail_tiles(n));
        for (uint32_t j = 0; j < w4_tail_chunks(n); ++j) { uint32_t cb, ce; w4_chunk_range(0, n, j, cb, ce); printf(" %u", ce - cb); }
        printf("\n");
    }
}
''')
    exe = tmp_path / "tails"
    subprocess.run([CXX, "-std=c++17", "-I", CSRC, "-o", str(exe), str(drv)], check=True, timeout=120)
    rows = [list(map(int, l.split())) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l]
    got = {r[0]: (r[1], r[2:]) for r in rows}
    assert got[51] == (3, [3]) and got[52] == (3, [3])
    assert got[54] == (3, [3]) and got[55] == (3, [3])
    assert got[87] == (5, [2, 3]) and got[88] == (5, [2, 3])
    assert got[127] == (7, [2, 2, 3]) and got[128] == (8, [2, 2, 2, 2])
    assert got[180] == (11, [2, 2, 2, 2, 3]) and got[181] == (11, [2, 2, 2, 2, 3])
