// search_plan.h -- the host decisions of one search: route, candidate count k', stage plan, the fast pass's error
// bound, the self-tuning candidate margin and the band-pass gate.  Plain arithmetic, no HIP headers: vrod_index.hip
// enqueues what these functions decide, and tests/test_search_plan.py compiles this header as host C++ and checks the
// decisions against the rules the tests state.  Whatever the environment or a kernel translation unit knows
// (VROD_DEBUG_*, the skinny kernel's capacity, the CU count) comes in as a parameter.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/vrod.h"

namespace vrod {

constexpr uint32_t kRowTile = 256;        // corpus capacity granularity (rows)
constexpr uint32_t kSelectChunk = 8192;   // select chunk capacity (kernels_select.hip); k' <= kSelectChunk / 2
// The kernels know two score forms: a dot product, higher is better (M_COSINE: COSINE and IP), and the squared L2
// distance (M_L2).
enum : int { M_COSINE = 0, M_L2 = 1 };

inline uint64_t round_up(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }

// The handle keeps the public metric; a kernel gets its score form, and preparation is told whether it normalises
// (M_COSINE) or only stores and rounds (M_L2: L2 and IP).  A raw VROD_METRIC_IP never reaches a kernel.
inline int score_form(int metric) { return metric == VROD_METRIC_L2 ? M_L2 : M_COSINE; }
inline int prep_form(int metric) { return metric == VROD_METRIC_COSINE ? M_COSINE : M_L2; }

// ------------------------------------------------------------------ route
// AUTO routing, measured on MI355X at 2M x 768 (scripts/probes/route_probe.py): the stream scan costs about one HBM pass
// per 8 queries (bf16: 0.63 / 0.69 / 2.0 ms at 1 / 4 / 8 queries, fp32: 1.09 / 1.21 / 1.47 / 2.85 ms at 1 / 4 / 8 / 16);
// an MFMA batch costs the same for any nq <= 256 (bf16 0.85 ms, fp32 5.97 ms: the fp32 MFMA rate is 16x lower).
// (opt-in split pass over an fp32 corpus: ~1.5 HBM passes + 3 bf16 MFMA products, cheaper than the stream scan from
// ~12 queries on; 5-32 queries over the planes take the skinny form where the queries' [hi | lo] fit in LDS: one HBM
// pass over the planes, 1.30 ms at 2M x 768 against 1.34-1.36 for a stream pass of 5-8 queries and 1.85 tiled)
struct Route {
    int path;      // VROD_PATH_STREAM / MFMA / EXACT
    bool split;    // the fast pass runs on the bf16 planes of the fp32 corpus (while the planes find room)
};
// The split pass is possible: enabled on an fp32 corpus, and its k' (k + max(32, k / 2)) fits the select windows.
inline bool can_split(bool split_enabled, int dtype, uint64_t N, uint32_t k) {
    return split_enabled && dtype == VROD_DTYPE_F32 && N > 0 && (uint64_t)k + std::max<uint32_t>(32, k / 2) <= kSelectChunk / 2;
}
// `forced` is the handle's path (VROD_PATH_AUTO or a forced one); `skinny_split_queries` the largest batch the skinny
// kernel takes over the planes (mfma_skinny_max_queries(true, planes row bytes)).
inline Route route(int forced, int dtype, bool split_enabled, uint32_t skinny_split_queries, uint64_t N, uint32_t nq, uint32_t k) {
    const bool split_ok = can_split(split_enabled, dtype, N, k);
    const bool skinny_split = split_ok && nq <= skinny_split_queries;
    int path = forced;
    if (path == VROD_PATH_AUTO)
        path = nq <= (dtype == VROD_DTYPE_BF16 ? 4u : skinny_split ? 4u : split_ok ? 12u : 32u) ? VROD_PATH_STREAM : VROD_PATH_MFMA;
    return {path, split_ok && path == VROD_PATH_MFMA};
}
// The route a search must have to be replayed from a graph (search_enqueue): the stream path forced, or AUTO with at
// most 4 queries.  Deliberately narrower than route(): fp32 batches of 5-8 queries take the stream path as well, but
// are not replayed.
inline bool graph_route(int forced, uint32_t nq) {
    return forced == VROD_PATH_STREAM || (forced == VROD_PATH_AUTO && nq <= 4);
}

// ------------------------------------------------------------------ filtered searches: dense scan or gather
// A handle with an allow-list filter (vrod_index_set_filter) has m eligible rows of its N.  The dense paths scan all N
// rows and drop the rest; the gather path (VROD_PATH_GATHER) computes the canonical score of the m eligible rows only
// (kernels_rescore.hip, the list form of rescore_all_kernel) -- no fast pass, no certificate, exact by construction.
// Both estimates are linear in the batch:
//   dense  = N * (row_bytes * kDenseNsPerByte + nq * dim * (kDenseNsPerStep[dtype] + kDenseNsPerMaskedStep * log10(N / m)))
//   gather = m * (row_bytes * kGatherNsPerByte + nq * dim * kGatherNsPerStep)
// The log term is what a narrow filter costs the batched scan: its thresholds are the k'-th best ELIGIBLE scores, which
// rows the filter drops beat too, and a dropped row's hit is dumped from the tile before the hit-log pass masks it.  The choice is
// monotone: gather at m = 0, dense at m = N, and a filter that is dense at (m, nq) stays dense for every larger m or nq
// (gather / dense grows with nq while kGatherNsPerStep * kDenseNsPerByte / kGatherNsPerByte exceeds the dense per-step
// cost, 1.0e-4 against at most 3e-6 + 3e-7 * log10(2^32)).
// Constants: MI355X, 10M x 768 bf16 cosine, k = 10, median ms per batch (scripts/probes/filter_probe.py,
// profiles/filter/README.md):
//   eligible            100 %   50 %    10 %    1 %     0.1 %   0.01 %
//   batch 1024 dense    11.54   11.71   12.51   16.41   26.05   36.63    (MFMA)
//   batch 1024 gather   -       623.9   121.6   12.28   1.436   0.241
//   batch 4 dense       2.885   2.922   2.912   2.691   2.526   2.484    (stream)
//   batch 4 gather      8.168   4.195   0.968   0.234   0.213   0.156
// dense: 2.9 ms per 15.4 GB pass -> 2.0e-4 ns per corpus byte; 11.5 - 2.9 ms over 10M x 1024 x 768 -> ~1.0e-6 ns per
// step on bf16 rows (an fp32 corpus: 3x, the split pass's three products); +4.9 / +14.5 / +25 ms at 1 / 0.1 / 0.01 %
// -> ~3e-7 ns per step and decade of N / m.  gather: 6.4e12 chain steps per second at batch 1024 -> 1.56e-4 ns per step;
// batch 4 at 10 % (0.97 ms, 1M rows) -> ~3.0e-4 ns per gathered row byte.
struct FilterCost { double dense_ns, gather_ns; };
constexpr double kDenseNsPerByte = 2.0e-4, kGatherNsPerByte = 3.0e-4;
constexpr double kDenseNsPerStepBf16 = 1.0e-6, kDenseNsPerStepF32 = 3.0e-6, kDenseNsPerMaskedStep = 3.0e-7;
constexpr double kGatherNsPerStep = 1.56e-4;
inline FilterCost filter_cost(int dtype, uint64_t N, uint64_t m, uint32_t nq, uint32_t dim) {
    const double row_bytes = (double)dim * (dtype == VROD_DTYPE_BF16 ? 2.0 : 4.0);
    const double steps = (double)nq * dim;
    const double masked = m > 0 && m < N ? std::log10((double)N / (double)m) : 0.0;
    const double dense_step = (dtype == VROD_DTYPE_BF16 ? kDenseNsPerStepBf16 : kDenseNsPerStepF32) + kDenseNsPerMaskedStep * masked;
    return {(double)N * (row_bytes * kDenseNsPerByte + steps * dense_step), (double)m * (row_bytes * kGatherNsPerByte + steps * kGatherNsPerStep)};
}
// Whether a search over m eligible rows of N takes the gather path.  `forced`: the handle's path -- GATHER always
// gathers, a forced dense path never does, AUTO compares the two estimates.
inline bool filter_route(int forced, int dtype, uint64_t N, uint64_t m, uint32_t nq, uint32_t dim) {
    if (forced == VROD_PATH_GATHER) return true;
    if (forced != VROD_PATH_AUTO) return false;
    if (m == 0) return true;
    const FilterCost c = filter_cost(dtype, N, m, nq, dim);
    return c.gather_ns < c.dense_ns;
}

// ------------------------------------------------------------------ k'
// Candidates per query the fast pass hands to the canonical re-score.  `kp_boost` is the handle's margin multiplier
// (KpBoost), `kp_margin` VROD_DEBUG_KP_MARGIN (0: the default 8).
inline uint32_t choose_kp(int path, bool split, int form, uint64_t N, uint32_t k, uint32_t kp_boost, uint32_t kp_margin) {
    if (split)   // the split pass's certificate bound is ~3x the fp32 MFMA pass's: more candidates per query
        return (uint32_t)std::min<uint64_t>(N, (uint64_t)k + std::max<uint32_t>(32, k / 2));
    if (path == VROD_PATH_MFMA) {
        // Every stage of the batched scan appends ~k' (g - 1) rows per query, and a hit costs its work-group ~0.35 us
        // (profiles/r02/mfma_experiments.md): fewer candidates, fewer hits.  The margin only has to keep the k-th
        // canonical score clear of the k'-th fast score by the error bound (1.8e-4 at d = 768 against ~8e-4 per rank at
        // 10M rows); margins 16 / 10 / 6 / 4 / 2 gave 0 / 0 / 0 / 11 / 937 failed certificates in 30 720 queries and
        // 12.58-12.65 / 12.53 / 12.51 / 13.27 / 15.44 ms per batch (1.25M-row shard: 1.82 / - / 1.75 / 1.80 ms); a failed
        // certificate costs a band pass, not a wrong result.  (The L2 bound through the norm expansion is ~4x wider
        // relative to the gaps: it keeps 16.  IP takes the dot-form margin: its bound is the same dot-form bound, scaled
        // by the real norms as its gaps are: rows with norms spread by exp(U(-1, 1)) failed no certificate at
        // 2M x 768, profiles/ip/.)
        const uint32_t margin = form == M_COSINE ? (kp_margin ? kp_margin : 8) : 16;
        return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(N, kSelectChunk / 2), (uint64_t)k + (uint64_t)std::max<uint32_t>(margin, k / 8) * kp_boost);
    }
    uint64_t kp = (uint64_t)k + std::max<uint32_t>(16, k / 8);   // stream (and exact) path
    if (kp > N) kp = N;
    if (kp > kSelectChunk / 2) kp = kSelectChunk / 2;
    return (uint32_t)kp;
}

// ------------------------------------------------------------------ the fast pass's error bound
// |fast - canonical| <= eps_bound(mode, c, max |q|^2, max |x|^2), formed by final_topk_kernel on the device (c goes
// there as it is: the expressions below keep their order and types, a different rounding could change which
// certificates pass):
//   mode 0  c |q| |x|        dot form (COSINE and IP: unit norms only for COSINE), stream and MFMA paths
//   mode 1  c (relative)     L2, stream path
//   mode 2  c (|q| + |x|)^2  L2 through the norm expansion, MFMA path
struct FastBound { int mode; float c; };
inline FastBound fast_bound(int path, bool split, int form, uint32_t dim) {
    const float u = 5.9604645e-8f;  // 2^-24
    FastBound b{0, 0.f};
    if (path == VROD_PATH_STREAM) {
        if (form == M_COSINE) b = {0, 4.f * dim * u};
        else b = {1, 4.f * (dim + 2) * u};
    } else if (path == VROD_PATH_MFMA) {
        if (form == M_COSINE) b = {0, 4.f * dim * u};
        else b = {2, 4.f * (dim + 4) * u};
        if (split) {
            // |fast - exact dot|: representation (x = hi + lo + r, |r| <= 2^-16 |x|, the lo.lo term dropped)
            // <= 3.1 * 2^-16 |q||x|; fp32 accumulation of 3*dim exact bf16 products in any order <= 4.1 * 3*dim * 2^-24
            // |q||x|.  (L2 = |q|^2 + |x|^2 - 2 q.x on the same dot.)
            const float repr = 3.1f * 1.52587890625e-5f;
            if (form == M_COSINE) b.c = 4.1f * 3.f * dim * u + repr;
            else b.c = 4.1f * (3.f * dim + 4) * u + repr;
        }
    }
    return b;
}
// The bound the search reports (vrod_search_stats::eps_bound) for the batch's largest |q|^2 and the corpus's largest |x|^2.
inline float eps_bound(int eps_mode, float eps_c, float qn2, float xn2) {
    const float qn = std::sqrt(qn2), xn = std::sqrt(xn2);
    return (eps_mode == 0 ? eps_c * qn * xn : eps_mode == 1 ? eps_c /* relative */ : eps_c * (qn + xn) * (qn + xn)) +
           (eps_mode == 1 ? 0.f : eps_c * 2.3509887e-38f);   // + the absolute slack of the denormal range
}

// ------------------------------------------------------------------ one search's plan
struct SearchPlan {
    int path = 0;
    bool split = false;      // the fast pass runs on the bf16 planes
    uint32_t kp = 0;         // candidates per query
    int eps_mode = 0;        // fast_bound()
    float eps_c = 0.f;
    uint32_t nq_pad = 0;     // queries padded to the fast pass's block (the list / counter / threshold blocks are sized by it)
    uint64_t N = 0;          // corpus rows
};
inline SearchPlan make_plan(int path, bool split, int form, uint32_t dim, uint64_t N, uint32_t nq, uint32_t k, uint32_t kp_boost,
                            uint32_t kp_margin) {
    SearchPlan p;
    p.path = path;
    p.split = split;
    p.kp = choose_kp(path, split, form, N, k, kp_boost, kp_margin);
    const FastBound b = fast_bound(path, split, form, dim);
    p.eps_mode = b.mode;
    p.eps_c = b.c;
    p.nq_pad = (uint32_t)round_up(nq, path == VROD_PATH_MFMA ? 256 : 8);
    p.N = N;
    return p;
}

// ------------------------------------------------------------------ stage plan of the MFMA path
// (DESIGN.md "Kernels").  Stage 0 is a DENSE sample (all scores of the first S rows written out, threshold = exact j-th
// best of them); every later stage is a filtered launch over g times more rows than everything before it, followed by a
// compaction (keep the best k', publish the k'-th score as the next threshold).  Each filtered stage thus expects about
// g*k' rows per query to beat its threshold: enough that a list cannot come up short, far too few to overflow it or to
// slow the scan.  `stage_growth` / `sample_rows`: VROD_DEBUG_STAGE_GROWTH / VROD_DEBUG_SAMPLE_ROWS (0: the defaults).
struct StagePlan { uint32_t S, j; std::vector<uint64_t> bounds; };
inline StagePlan plan_stages(uint64_t N, uint32_t kp, uint32_t cap, uint32_t max_sample_rows, uint64_t stage_growth,
                             uint64_t sample_rows) {
    StagePlan p;
    // Growth per filtered stage.  A stage over rows (b, g*b] runs against the k'-th best of the
    // first b rows, so about k'*(g-1) rows per query beat its threshold: that must stay well under
    // the list capacity, and -- measured -- appends are not free: the first stage after the
    // 16K-row sample appends one row in 630 per query (~100 per 256x256 tile) and runs at 1.9 us
    // per 1000 rows against 1.3 once appends are rare.  The extra time of a stage is ~ (g-1), the
    // number of stages ~ 1/ln g, each costing a launch ramp and a compaction (~40 us): the total is
    // flat between g = 4 and 8 and twice as large at g = 25 (two stages at 10M rows: tried,
    // +0.25 ms per batch).
    // Round 2, same box, batch 1024 x 768 (profiles/r02/mfma_experiments.md): 10M rows, g = 3 / 4 / 5 / 6 / 8 -> 12.69 / 12.70 /
    // 12.70 / 12.75 / 12.77-12.87 ms per batch; with the candidate margin at 8, 5M rows g = 4 / 5 / 6 / 8 -> 6.47 / 6.41 / 6.48 /
    // 6.49, 2.5M -> 3.24 / 3.26 / 3.27 / 3.25, 1.25M -> 1.759 / 1.755 / 1.757 / 1.790.  What a stage pays per hit is the OTHER
    // three waves of the work-group waiting at the next barrier for the wave that walks a hit column (~0.35 us of
    // work-group time per append, not 0.1), against ~40 us of ramp + compaction per extra stage: g = 5 at every size.
    const uint64_t g_auto = 5;
    const uint64_t g = std::max<uint64_t>(2, std::min<uint64_t>(stage_growth ? stage_growth : g_auto, cap / (3ull * kp)));
    // sample: N/g^2 rows, at most one round of work-groups (one 256-row tile per work-group of
    // the dense launch)
    if (sample_rows) max_sample_rows = (uint32_t)std::min<uint64_t>(sample_rows, max_sample_rows);
    uint64_t S = std::min<uint64_t>(N / (g * g), max_sample_rows);
    S = std::max<uint64_t>(S, std::min<uint64_t>(N, std::max<uint64_t>(4ull * kp, kRowTile)));
    S = std::min<uint64_t>(round_up(S, kRowTile), N);
    p.S = (uint32_t)S;
    p.j = (uint32_t)std::min<uint64_t>(kp, S);
    for (uint64_t b = S * g; b < N; b *= g) {
        if (N - b < b / 2) break;                    // the tail would be a sliver: fold it in
        p.bounds.push_back(b / kRowTile * kRowTile);
    }
    p.bounds.push_back(N);
    return p;
}

// ------------------------------------------------------------------ self-tuning candidate margin
// Of the batched scan without the split pass: k' = k + margin * boost.  A failed certificate costs a band pass (one
// more scan of the corpus); doubling the margin costs a few per cent of hits.  The boost doubles (up to 8) after a
// search with failures, halves after 64 clean ones; failures AT 8 mean the margin is not what those queries lack
// (exact duplicates): back to 1 and left alone for 256 searches.
struct KpBoost {
    static constexpr uint32_t kMax = 8;
    uint32_t boost = 1, clean = 0, hold = 0;
};
// The verdict of a completed search that ran with multiplier `used` (two searches may be in flight: a verdict counts
// only for the multiplier the search itself ran with).
inline void kp_boost_step(KpBoost& s, uint32_t used, bool failures) {
    if (s.hold) --s.hold;
    if (failures) {
        s.clean = 0;
        if (used >= KpBoost::kMax) { s.boost = 1; s.hold = 256; }
        else if (!s.hold && used == s.boost) s.boost *= 2;
    } else if (used == s.boost && ++s.clean >= 64 && s.boost > 1) {
        s.boost /= 2;
        s.clean = 0;
    }
}
// Whether a completed search's verdict moves the margin at all.
inline bool kp_boost_applies(const SearchPlan& p, uint32_t nq) { return p.path == VROD_PATH_MFMA && !p.split && nq; }

// ------------------------------------------------------------------ band pass gate
// From how many failed queries on the band pass beats the exact path.  On bf16 rows (or the bf16 planes of an fp32
// corpus) a band pass of <= 64 queries is the skinny kernel, ONE HBM-bound pass over the corpus (2.8 ms at 15.4 GB),
// while the exact path's pass of 8 queries is VALU-bound (9 ms there; cfg3dup, 8 failed queries per batch: 22.2 ms
// per batch through the exact path, 15.9 through the band pass): from 2 queries on.  An fp32 corpus without planes
// scans at the fp32 matrix rate (16x lower), several exact passes long: only for batches of failures.
constexpr uint32_t kBandMinQueriesFast = 2, kBandMinQueriesF32 = 48;
// The band needs the MFMA path's list block and a bound in absolute terms (not the stream path's relative L2 mode).
inline bool band_eligible(const SearchPlan& p, int dtype, uint32_t n_failed, uint32_t k) {
    const uint32_t min_q = (dtype == VROD_DTYPE_BF16 || p.split) ? kBandMinQueriesFast : kBandMinQueriesF32;
    return p.path == VROD_PATH_MFMA && p.eps_mode != 1 && n_failed >= min_q && p.N >= k && p.nq_pad != 0;
}

// ------------------------------------------------------------------ range searches
// A range search (vrod_range_search) returns every eligible row whose canonical score is at least as good as the
// caller's threshold.  Its fast pass is ONE filtered MFMA launch per row range at a threshold widened by the error
// bound; the canonical re-score of what it collected decides membership.  Nothing is estimated: no sample pass, no
// stages, no k', no certificate.
#if defined(__HIPCC__)
#define VROD_PLAN_HD __host__ __device__
#else
#define VROD_PLAN_HD
#endif
// The next float on the WORSE side of t (form M_COSINE: below, M_L2: above); t finite.
VROD_PLAN_HD inline float range_step_worse(float t, int form) {
    union { float f; uint32_t u; } v;
    v.f = t;
    const bool down = form == M_COSINE;
    if ((v.u & 0x7FFFFFFFu) == 0u) v.u = (down ? 0x80000000u : 0u) | 1u;       // +-0 -> the smallest denormal of that side
    else if (((v.u >> 31) != 0u) == down) v.u += 1u;                            // away from zero
    else v.u -= 1u;                                                             // towards zero
    return v.f;
}
// The fast-pass threshold of one query.  The scan appends rows whose fast score is STRICTLY better than it; with
// |fast - canonical| <= eps every row whose canonical score is at least as good as `threshold` has a fast score at
// least as good as threshold -/+ eps, and the rounded difference moved one float further is strictly worse than
// that: the lists are a superset of the answer, equality included.  eps is eps_bound()'s expression for the batch's
// largest |q|^2 and the corpus's largest |x|^2.  An infinite threshold stays as it is: on the permissive side every
// finite fast score passes, on the other nothing does.  *canonical is set when no finite bound exists (a NaN or
// overflowing norm product -- the IP and overflowing-L2 cases -- or the relative mode 1, which has no absolute form):
// that query must take the canonical route, and its fast threshold lets nothing pass.
VROD_PLAN_HD inline float range_fast_threshold(float threshold, int form, int eps_mode, float eps_c, float qn2, float xn2, bool* canonical) {
    const float kMax = 3.4028234663852886e38f, kInf = __builtin_huge_valf();
    const float never = form == M_COSINE ? kInf : -kInf;
    const float qn = __builtin_sqrtf(qn2), xn = __builtin_sqrtf(xn2);
    const float span = eps_mode == 0 ? qn * xn : (qn + xn) * (qn + xn);
    const float eps = eps_c * span + eps_c * 2.3509887e-38f;
    *canonical = eps_mode == 1 || !(span <= kMax) || !(span + eps <= kMax);
    if (*canonical) return never;
    if (threshold == kInf || threshold == -kInf) return threshold;
    const float t = form == M_COSINE ? threshold - eps : threshold + eps;
    if (!(__builtin_fabsf(t) <= kMax)) return t;   // overflowed to the permissive infinity (a threshold within eps of FLT_MAX)
    return range_step_worse(t, form);
}

// Split policy of the filtered launches.  A launch over rows [lo, hi) found max_count hits for its fullest query
// against a list capacity of cap: more than cap means the range is redone in pieces.  The pieces are whole 256-row
// tiles (the last one ends at hi), cover [lo, hi) exactly once, and number ceil(max_count / (cap / 2)) -- at least 2,
// at most the range's tiles -- so that a piece expects half a list.  A range of one tile is never split: a tile
// appends at most 256 rows per query.  Returns the pieces' bounds: piece i is [b[i], b[i + 1]).
inline std::vector<uint64_t> range_split(uint64_t lo, uint64_t hi, uint64_t max_count, uint32_t cap) {
    const uint64_t t0 = lo / kRowTile, t1 = (hi + kRowTile - 1) / kRowTile;
    const uint64_t tiles = t1 > t0 ? t1 - t0 : 0;
    std::vector<uint64_t> b{lo};
    if (tiles > 1 && max_count > cap) {
        const uint64_t half = std::max<uint64_t>(cap / 2, 1);
        const uint64_t pieces = std::min<uint64_t>(tiles, std::max<uint64_t>(2, (max_count + half - 1) / half));
        for (uint64_t i = 1; i < pieces; ++i) b.push_back((t0 + tiles * i / pieces) * kRowTile);
    }
    b.push_back(hi);
    return b;
}
// The fast pass a range search runs: always the batched scan (it is the one with a threshold form); over the bf16
// planes on an fp32 handle that has them.
inline SearchPlan make_range_plan(bool split, int form, uint32_t dim, uint64_t N, uint32_t nq) {
    SearchPlan p;
    p.path = VROD_PATH_MFMA;
    p.split = split;
    p.kp = 0;
    const FastBound fb = fast_bound(VROD_PATH_MFMA, split, form, dim);
    p.eps_mode = fb.mode;
    p.eps_c = fb.c;
    p.nq_pad = (uint32_t)round_up(nq, 256);
    p.N = N;
    return p;
}

}  // namespace vrod
