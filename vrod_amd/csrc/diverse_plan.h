// diverse_plan.h -- the host decisions of a diversified search (vrod_search_diverse): the checks the arguments alone
// decide, and the LDS arithmetic of the selection kernel (kernels_diverse.hip) -- how many waves, hence chain tiles, one
// work-group gets at a given row width and pool.  Plain arithmetic, no HIP headers (search_plan.h, multivec_plan.h):
// vrod_index.hip and kernels_diverse.hip use what these functions decide, tests/test_diverse_plan.py compiles this
// header as host C++.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace vrod {

// The largest pool of the ABI (VROD_MAX_DIVERSE_POOL) and the widest row (VROD_MAX_DIM).
constexpr uint32_t kDiverseMaxPool = 1024;
constexpr uint32_t kDiverseMaxDim = 32768;

// 0: fine; 1: k == 0; 2: k > pool; 3: pool > kDiverseMaxPool; 4: lambda is NaN or outside [0, 1].
inline int diverse_check_args(uint32_t k, uint32_t pool, float lambda) {
    if (k == 0) return 1;
    if (k > pool) return 2;
    if (pool > kDiverseMaxPool) return 3;
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return 4;
    return 0;
}

// ---- the selection kernel's LDS, in bytes, in this order:
//   the selected row, widened to fp32      round_up(dim, 4) floats (the chain reads whole groups of four)
//   one chain tile per wave                64 rows x kTileStride (68) dwords (rescore_chain.h)
//   the arg-best exchange                  one 64-bit key per wave (kDiverseMaxWaves of them)
//   the taken bits, the control words      kDiverseMaxPool / 8 bytes, four words
//   per pool position                      local row, r, pen: three words
constexpr uint32_t kDiverseLdsCap = 160u * 1024u;
constexpr uint32_t kDiverseTileBytes = 64u * 68u * 4u;
// (four waves, one per SIMD: the fp32 chain keeps three chunks of 64 rows in flight and wants the whole register file)
constexpr uint32_t kDiverseMaxWaves = 4;
constexpr uint32_t kDiverseFixedBytes = kDiverseMaxPool / 8 + kDiverseMaxWaves * 8 + 16;

// (constexpr: the kernel calls it too)
constexpr uint32_t diverse_row_floats(uint32_t dim) { return (dim + 3u) & ~3u; }
inline uint32_t diverse_lds_bytes(uint32_t dim, uint32_t pool, uint32_t waves) {
    return diverse_row_floats(dim) * 4u + waves * kDiverseTileBytes + pool * 12u + kDiverseFixedBytes;
}
// Waves of one work-group: one per 64 pool positions (a wave scores 64 positions per chain pass), at most
// kDiverseMaxWaves, and no more than the tiles that fit beside the row; 0: not even one fits (no dim <= kDiverseMaxDim
// with a pool <= kDiverseMaxPool gets there).
inline uint32_t diverse_waves(uint32_t dim, uint32_t pool) {
    uint32_t w = std::min<uint32_t>(kDiverseMaxWaves, std::max<uint32_t>(1u, (pool + 63u) / 64u));
    while (w && diverse_lds_bytes(dim, pool, w) > kDiverseLdsCap) --w;
    return w;
}

}  // namespace vrod
