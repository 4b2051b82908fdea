// label_plan.h -- the host decisions of a labelled search (vrod_search_labeled): the batch's queries grouped by their
// label, and the work table of the segmented score launch.  Plain arithmetic, no HIP headers (search_plan.h,
// compact_plan.h): vrod_index.hip enqueues what these functions decide, tests/test_label_plan.py compiles this header as
// host C++.  seg_lookup is the one function the score kernel shares with the host (kernels_rescore.hip).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define VROD_LABEL_HD __host__ __device__
#else
#define VROD_LABEL_HD
#endif

namespace vrod {

// Distinct labels one grouping pass serves (kernels_label.hip keeps the sorted table and one counter per label in LDS);
// a batch with more is served in passes of this many groups.
constexpr uint32_t kLabelGroupsPerPass = 4096;
// A group's entry in the offsets the scatter pass gets: this group needs no row list (it takes the dense route).
constexpr uint32_t kNoSegment = 0xFFFFFFFFu;

// ------------------------------------------------------------------ grouping
// The batch's distinct satisfiable predicates in ascending order, and per predicate its queries in ascending order:
// group g is q_order[q_off[g] .. q_off[g + 1]).  The queries of unsatisfiable predicates come last in q_order, from
// q_off[size()] on, ascending: they belong to no group and no pass, their result rows are all unfilled.
// (A template over the predicate: a label here, tag_plan.h's and where_plan.h's wider ones.)
template <typename Pred>
struct PredGroups {
    std::vector<Pred> preds;         // [G]
    std::vector<uint32_t> q_off;     // [G + 1]
    std::vector<uint32_t> q_order;   // [nq]
    uint32_t size() const { return (uint32_t)preds.size(); }
    uint32_t nq_of(uint32_t g) const { return q_off[g + 1] - q_off[g]; }
    uint32_t n_unsatisfiable() const { return (uint32_t)q_order.size() - q_off.back(); }
};
// unsat(p): no row can match p; before(a, b): the strict order of the groups.
template <typename Pred, typename Unsat, typename Before>
inline PredGroups<Pred> group_preds(const Pred* p, uint32_t nq, Unsat unsat, Before before) {
    PredGroups<Pred> G;
    G.q_order.resize(nq);
    for (uint32_t i = 0; i < nq; ++i) G.q_order[i] = i;
    auto less = [&](uint32_t a, uint32_t b) {
        const bool ua = unsat(p[a]), ub = unsat(p[b]);
        if (ua != ub) return ub;
        if (ua) return false;
        return before(p[a], p[b]);
    };
    std::stable_sort(G.q_order.begin(), G.q_order.end(), less);
    uint32_t i = 0;
    for (; i < nq && !unsat(p[G.q_order[i]]); ++i) {
        const Pred& t = p[G.q_order[i]];
        if (G.preds.empty() || before(G.preds.back(), t)) {
            G.preds.push_back(t);
            G.q_off.push_back(i);
        }
    }
    G.q_off.push_back(i);
    return G;
}
// Labels: every label can occur, so every query is in a group; ascending.  `labels` is the groups' `preds` under the
// name a label's readers use (a reference into the object itself, so the object is built in place and never copied).
struct LabelGroups : PredGroups<uint32_t> {
    const std::vector<uint32_t>& labels = preds;   // [G]
    LabelGroups(PredGroups<uint32_t>&& g) : PredGroups<uint32_t>(std::move(g)) {}
    LabelGroups(const LabelGroups&) = delete;
};
inline LabelGroups label_groups(const uint32_t* query_labels, uint32_t nq) {
    return group_preds(query_labels, nq, [](uint32_t) { return false; }, [](uint32_t a, uint32_t b) { return a < b; });
}

// Rows per block of the grouping pass over N rows: whole 64-row waves, about 2048 blocks on a large corpus (each block's
// per-group counts are one row of the [blocks][groups] matrix the prefix pass walks).
inline uint32_t label_rows_per_block(uint64_t N) {
    return (uint32_t)std::max<uint64_t>(256, ((N + 2047) / 2048 + 63) / 64 * 64);
}

// ------------------------------------------------------------------ the segmented score launch
// A segmented group: `nq` queries, in score slots [slot0, slot0 + nq), over the `m` rows of its segment of the list
// buffer.  Slots number the queries of the segmented groups only, group after group.
struct SegGroup { uint32_t list_base, m, slot0, nq; };
// The segmented groups of one pass as plan_segments and the score launch take them, group after group: slot s is query
// slot_q[s] over the slot_len[s] list entries from slot_base[s] on.
struct SlotTables {
    std::vector<SegGroup> segs;
    std::vector<uint32_t> slot_q, slot_len, slot_base;
    uint32_t size() const { return (uint32_t)slot_q.size(); }
    // a group of `nq` queries over the `m` rows of the list buffer from `list_base` on: the next `nq` slots
    void add(uint32_t list_base, uint32_t m, const uint32_t* queries, uint32_t nq) {
        segs.push_back({list_base, m, size(), nq});
        slot_q.insert(slot_q.end(), queries, queries + nq);
        slot_len.insert(slot_len.end(), nq, m);
        slot_base.insert(slot_base.end(), nq, list_base);
    }
};
// Queries per lane a group's blocks take (the NQ of rescore_all_body): 8 once the group has 5, so that a group's last
// subgroup never needs a second kernel form.
VROD_LABEL_HD inline uint32_t seg_query_class(uint32_t nq) { return nq >= 5 ? 8u : nq >= 3 ? 4u : nq; }
// One entry of the device work table: blocks [block0, block0 + tiles * subgroups) of the launch, block0 + t * subgroups
// + s = (tile t, subgroup s) -- the subgroups of one tile are neighbours.  Entries have m > 0 and ascending block0.
struct SegEntry { uint32_t block0, list_base, m, slot0, nq, nqc; };
VROD_LABEL_HD inline uint32_t seg_subgroups(const SegEntry& e) { return (e.nq + e.nqc - 1) / e.nqc; }
VROD_LABEL_HD inline uint32_t seg_tiles(const SegEntry& e) { return (e.m + 63) / 64; }
struct SegBlock { uint32_t entry, sub, tile; };
VROD_LABEL_HD inline SegBlock seg_lookup(const SegEntry* e, uint32_t n, uint32_t b) {
    uint32_t lo = 0, hi = n;   // the last entry with block0 <= b
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (e[mid].block0 <= b) lo = mid; else hi = mid;
    }
    const uint32_t local = b - e[lo].block0, ns = seg_subgroups(e[lo]);
    return {lo, local % ns, local / ns};
}
// One launch: entries [e0, e1) of the table (block0 relative to the launch), the slots [slot0, slot0 + n_slots) whose
// scores it writes, as [n_slots][out_ld] with out_ld = the longest segment rounded up to 64 columns.
struct SegChunk { uint32_t e0, e1, slot0, n_slots, n_blocks, max_m; };
struct SegPlan {
    std::vector<SegEntry> entries;
    std::vector<SegChunk> chunks;
};
// Chunks of whole entries whose score block stays under `max_bytes` (the 1 GiB rule of the gather and exact paths); a
// group whose own block would not fit is cut into entries of a multiple of 8 queries (8 at the least).  Every slot
// belongs to exactly one chunk, groups with m == 0 included: they have no entry and no block, their queries' rows of
// the score block are never read (the select's per-query length is 0).
inline SegPlan plan_segments(const std::vector<SegGroup>& groups, uint64_t max_bytes = 1ull << 30) {
    SegPlan P;
    SegChunk c{0, 0, 0, 0, 0, 0};
    auto bytes = [](uint64_t slots, uint64_t m) { return slots * ((std::max<uint64_t>(m, 1) + 63) / 64 * 64) * 4; };
    auto close = [&] {
        c.e1 = (uint32_t)P.entries.size();
        if (c.n_slots) P.chunks.push_back(c);
        c = SegChunk{c.e1, c.e1, c.slot0 + c.n_slots, 0, 0, 0};
    };
    for (const SegGroup& g : groups) {
        const uint64_t fit = max_bytes / bytes(1, g.m);
        const uint32_t piece = (uint32_t)std::min<uint64_t>(g.nq, std::max<uint64_t>(8, fit / 8 * 8));
        for (uint32_t q0 = 0; q0 < g.nq; q0 += piece) {
            const uint32_t nq = std::min(piece, g.nq - q0);
            if (c.n_slots && bytes(c.n_slots + nq, std::max(c.max_m, g.m)) > max_bytes) close();
            if (g.m) {
                SegEntry e{c.n_blocks, g.list_base, g.m, g.slot0 + q0, nq, seg_query_class(nq)};
                c.n_blocks += seg_tiles(e) * seg_subgroups(e);
                P.entries.push_back(e);
            }
            c.n_slots += nq;
            c.max_m = std::max(c.max_m, g.m);
        }
    }
    close();
    return P;
}

}  // namespace vrod
