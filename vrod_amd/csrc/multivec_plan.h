// multivec_plan.h -- the host decisions of a multi-vector search (vrod_search_multivec): the checks of query_lims, how
// many results the first-stage search asks for per vector, where a call is cut into sub-batches, when the candidate
// route's answer is certified, and when a query is sent to the dense route instead.  Plain arithmetic, no HIP headers
// (search_plan.h, group_plan.h): vrod_index.hip enqueues what these functions decide, tests/test_multivec_plan.py
// compiles this header as host C++.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace vrod {

// The largest k of the ABI (VROD_MAX_K) and the most vectors one query may hold (VROD_MAX_QUERY_VECTORS).
constexpr uint32_t kMultivecMaxK = 3584;
constexpr uint32_t kMultivecMaxVectors = 256;
// Vectors one first-stage search carries: a call with more is cut between queries.  A query holds at most
// kMultivecMaxVectors, so a sub-batch always takes at least one whole query.
constexpr uint32_t kMultivecBatchVectors = 2048;

// query_lims: nq + 1 words, lims[0] == 0, non-decreasing, every query 1 .. kMultivecMaxVectors vectors.
// 0: fine; 1: lims[0] != 0; 2: decreasing; 3: a query without a vector; 4: a query with too many.
inline int multivec_check_lims(const uint32_t* lims, uint32_t nq) {
    if (lims[0] != 0) return 1;
    for (uint32_t q = 0; q < nq; ++q) {
        if (lims[q + 1] < lims[q]) return 2;
        if (lims[q + 1] == lims[q]) return 3;
        if (lims[q + 1] - lims[q] > kMultivecMaxVectors) return 4;
    }
    return 0;
}

// Results per vector the first-stage search asks for: the grouped search's rule (group_plan.h group_first_k) -- four
// times k, at least k + 32, never more than the ABI's largest k or the eligible rows.  0 without an eligible row.
inline uint32_t multivec_first_k(uint32_t k, uint64_t eligible) {
    const uint64_t rule = std::max<uint64_t>(4ull * k, (uint64_t)k + 32);
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(kMultivecMaxK, eligible), rule);
}

// The sub-batch that starts at query q0: queries [q0, q1) with q1 the largest end whose vectors, lims[q1] - lims[q0],
// stay within max_vectors -- and at least one query (lims passed multivec_check_lims).
inline uint32_t multivec_cut(const uint32_t* lims, uint32_t nq, uint32_t q0, uint32_t max_vectors = kMultivecBatchVectors) {
    uint32_t q1 = q0 + 1;
    while (q1 < nq && lims[q1 + 1] - lims[q0] <= max_vectors) ++q1;
    return q1;
}

// The candidate route's certificate.  theta_t = the last entry of vector t's full list: a label none of whose rows is
// in that list has M(t, L) no better than theta_t, and rounded addition is monotone, so U = the fl-sum of theta_t in
// vector order bounds S of every non-candidate label.  The k best candidates are final when there are k of them and the
// k-th S is STRICTLY better than U (equal: a non-candidate with a smaller label could tie and win); a NaN on either side
// certifies nothing.  `complete`: one of the query's lists came back short, or the lists are as long as the eligible
// rows -- then every label with an eligible row is a candidate and the candidates' ranking is final as it is.
// better_is_higher: COSINE and IP; else L2.
inline bool multivec_certified(bool complete, uint32_t n_candidates, uint32_t k, float kth_score, float U, bool better_is_higher) {
    if (complete) return true;
    if (n_candidates < k) return false;
    return better_is_higher ? kth_score > U : kth_score < U;
}
inline bool multivec_lists_complete(bool any_short, uint32_t k1, uint64_t eligible) { return any_short || k1 >= eligible; }

// A query whose candidate labels own more than 1/kMultivecDenseShare of the stored rows is answered by the dense
// route: scoring that many rows per vector through the row lists costs more than the dense pass over the corpus.
constexpr uint64_t kMultivecDenseShare = 4;
inline bool multivec_candidates_too_broad(uint64_t candidate_rows, uint64_t stored_rows) {
    return candidate_rows * kMultivecDenseShare > stored_rows;
}
// Score slots -- (candidate label, vector) pairs -- one sub-batch may hold on the candidate route: the queries that would
// take it past this go dense (one fp32 word per slot, and a row of the score block while its chunk is scored).
constexpr uint64_t kMultivecMaxSlots = 1ull << 26;
// There is no retry with a longer list: a query that is not certified goes to the dense route at once.

// De-duplication table of one query (kernels_multivec.hip): a power of two of slots, at least twice its list entries.
inline uint32_t multivec_table_slots(uint32_t entries) {
    uint32_t s = 64;
    while (s < 2 * entries) s <<= 1;
    return s;
}
// What that kernel gets per query: its vectors [v0, v0 + m) of the sub-batch (m * k1 list entries), where its entry
// labels / candidate labels (ent_off) and its table (tab_off, `slots` slots, hash = (label * c) >> shift) start.
struct MultivecQuery { uint32_t v0, m, ent_off, tab_off, slots, shift; };

}  // namespace vrod
