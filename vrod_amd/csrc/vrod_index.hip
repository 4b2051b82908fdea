// vrod_index.hip -- the index object and the C ABI of libvrod_hip.so (include/vrod.h).
//
// This is the corpus owner vRod's `Database` never got (reference src/database/mod.rs:6-10:
// "//TODO collections") and the body SearchSimilarCommand::execute never got
// (src/command/types.rs:127-132).  Pipeline of one search (DESIGN.md "Pipeline"):
//
//   prepare queries -> FAST PASS (stream scan | MFMA scan with threshold filter)
//     -> k' candidates per query + T (bound on the fast score of everything left out)
//     -> canonical re-score of the candidates (oracle order, bit-exact)
//     -> final ordering by (canonical score, id) + exactness certificate
//     -> queries whose certificate fails take the EXACT path (canonical scan of all rows)
//
// so the returned ids and score bits are identical to the CPU oracle's for every input.
// There is no CPU fallback anywhere: without a gfx950 device every entry point fails.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is dlopen'ed when a multi-device handle is created

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vrod.h"
#include "vrod_common.h"
#include "vrod_kernels.h"
#include "kernels_range.h"
#include "search_plan.h"
#include "compact_plan.h"
#include "label_plan.h"
#include "tag_plan.h"
#include "where_plan.h"
#include "dup_plan.h"
#include "near_plan.h"
#include "group_plan.h"
#include "multivec_plan.h"
#include "diverse_plan.h"
#include "byid_plan.h"
#include "combine_plan.h"
#include "snapshot_plan.h"
#include "keys_plan.h"
#include "ingest_plan.h"
#include "rowfind_plan.h"

using namespace vrod;

static_assert(kGroupMaxK == VROD_MAX_K, "group_plan.h restates the largest k of the ABI");
static_assert(kByidMaxK == VROD_MAX_K, "byid_plan.h restates the largest k of the ABI");
static_assert(kMultivecMaxK == VROD_MAX_K && kMultivecMaxVectors == VROD_MAX_QUERY_VECTORS, "multivec_plan.h restates the ABI's limits");
static_assert(kCombineMaxK == VROD_MAX_K && kCombineMaxTerms == VROD_MAX_COMBINE_TERMS && kCombineMaxExclude == VROD_MAX_EXCLUDE &&
                  kCombineExcludeTerms == VROD_COMBINED_EXCLUDE_TERMS,
              "combine_plan.h restates the ABI's limits");
static_assert(kKeyNone == VROD_ID_NONE, "keys_plan.h restates the ABI's \"no key\"");
static_assert(kDiverseMaxPool == VROD_MAX_DIVERSE_POOL && kDiverseMaxPool <= VROD_MAX_K && kDiverseMaxDim == VROD_MAX_DIM,
              "diverse_plan.h restates the ABI's limits");

// ------------------------------------------------------------------ errors
static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? VROD_ERR_OUT_OF_MEMORY : VROD_ERR_HIP,     \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,       \
                        __LINE__);                                                             \
    } while (0)

#define VROD_TRY(expr)              \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != VROD_OK) return rc_; \
    } while (0)

// ------------------------------------------------------------------ device buffer that only grows
// It owns its memory: whatever holds one (the handle, a Pending, a DevGroup) frees it by going away, under the device
// that is current then, and cannot be copied.  A buffer on another device than its holder's is released by hand first.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return VROD_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(VROD_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return VROD_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return (T*)p; }
};

// ------------------------------------------------------------------ device block of a fixed size
// What is sized by the capacity (the corpus, the norms, the bitmaps, the row columns) or once and for all (the flag words,
// the key table) lives in one of these: exactly the bytes asked for, and never freed before its replacement exists --
// alloc() on a block that holds memory lets go of it only once the new memory is there, and whoever needs two blocks
// replaced together builds them in locals and swaps them in.  Owned as a DevBuf is: freed by going away, not copyable.
template <typename T = void>
struct DevMem {
    T* p = nullptr;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    DevMem(DevMem&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) { release(); p = o.p; o.p = nullptr; }
        return *this;
    }
    ~DevMem() { release(); }
    hipError_t alloc(size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        release();
        p = (T*)q;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    void swap(DevMem& o) noexcept { std::swap(p, o.p); }
    template <typename U> U* get() const { return (U*)p; }
};

// ------------------------------------------------------------------ a per-row word column (labels, tags, values, keys)
// One word of type T per row of the capacity: a host mirror, which is the truth for the getters, and a device copy, which
// is what the kernels read.  Neither exists before the first set: until then, and for rows at or beyond the count, every
// row carries `none` (all bytes 0x00, or all bytes 0xFF), and a handle that never set one allocates nothing for it.
// Growth and compaction are staged -- everything that can fail -- and committed later by steps that cannot.
using ColumnBytes = std::vector<unsigned char>;   // a staged compaction's rows, whatever the column's word is
template <typename T>
struct RowColumn {
    std::vector<T> host;       // [capacity] once the column exists
    DevMem<> dev;              // [capacity] on the device, or empty
    const T none;
    const char* const noun;    // "labels": for messages
    const uint32_t snap_kind;  // its section in a snapshot (snapshot_plan.h)
    RowColumn(T none_, const char* noun_, uint32_t kind) : none(none_), noun(noun_), snap_kind(kind) {}

    bool exists() const { return dev.p != nullptr; }
    T* d() const { return dev.get<T>(); }
    int fill_byte() const { return none == T(0) ? 0 : 0xFF; }
    T get(uint64_t r) const { return exists() ? host[r] : none; }

    // the first set of the handle: every row carries `none` so far
    int create(uint64_t capacity) {
        DevMem<> fresh;
        HIP_TRY(fresh.alloc(capacity * sizeof(T)));
        const hipError_t e = hipMemset(fresh.p, fill_byte(), capacity * sizeof(T));
        if (e != hipSuccess) return fail(VROD_ERR_HIP, "clearing the row %s: %s", noun, hipGetErrorString(e));
        dev.swap(fresh);
        host.assign(capacity, none);
        return VROD_OK;
    }
    // rows [r0, r0 + n) take src[0 .. n): the device copy, then the mirror
    int set(uint64_t r0, const T* src, uint64_t n) {
        HIP_TRY(hipMemcpy(d() + r0, src, n * sizeof(T), hipMemcpyHostToDevice));
        std::copy(src, src + n, host.begin() + r0);
        return VROD_OK;
    }

    // Growth to `want` rows, staged: `grown` gets a block holding rows [0, count) of the mirror and `none` above them,
    // filled on `s` (the caller drains it).  Nothing of the column changes; a column that does not exist stages nothing.
    hipError_t stage_grow(uint64_t count, uint64_t want, hipStream_t s, DevMem<>& grown) const {
        if (!exists()) return hipSuccess;
        hipError_t e = grown.alloc(want * sizeof(T));
        if (e == hipSuccess) e = hipMemsetAsync(grown.p, fill_byte(), want * sizeof(T), s);
        if (e == hipSuccess) e = hipMemcpyAsync(grown.p, host.data(), count * sizeof(T), hipMemcpyHostToDevice, s);
        return e;
    }
    // ... and committed: the staged block comes in, `grown` leaves with the old one
    void commit_grow(uint64_t want, DevMem<>& grown) {
        if (!exists()) return;
        dev.swap(grown);
        host.resize(want, none);
    }

    // Compaction under the tombstones `del`, staged: rows [0, count) as they will stand (compact_plan.h compact_column);
    // then uploaded on `s`, then taken over by the mirror.  A column that does not exist takes part in none of the three.
    void stage_compact(const uint32_t* del, uint64_t count, ColumnBytes& moved) const {
        if (!exists()) return;
        moved.resize(count * sizeof(T));
        compact_column(del, host.data(), count, none, (T*)moved.data());
    }
    hipError_t upload_compact(const ColumnBytes& moved, hipStream_t s) {
        return exists() ? hipMemcpyAsync(dev.p, moved.data(), moved.size(), hipMemcpyHostToDevice, s) : hipSuccess;
    }
    void commit_compact(const ColumnBytes& moved) {
        if (exists()) memcpy(host.data(), moved.data(), moved.size());
    }
};

// a search slot's block of device words: 64 scalars, then one region of sibling-pacing counters and one of work-stealing
// claim bits per scan launch of the search (8 of each; a search with more launches reuses them behind a memset)
constexpr uint32_t kPaceRegions = 8, kPaceWords = 192, kClaimWords = (uint32_t)kMfmaClaimWords;
constexpr size_t kSlotFlagBytes = (64 + kPaceRegions * (kPaceWords + kClaimWords)) * 4;

// ------------------------------------------------------------------ one search in flight
// A search is ENQUEUED (every launch up to the D2H of its status block) and later COMPLETED (wait
// for that copy, read the certificate's verdicts, run the exact path for the rare failures).  Two
// slots let the caller enqueue search s+1 before it completes search s, so the device never waits
// for the host between batches and the caller's exchange of batch s (all-gather + merge on its own
// stream) overlaps the scan of batch s+1.
struct Pending {
    bool active = false;
    bool trivial = false;          // nq == 0 or empty corpus: the outputs are already final
    uint32_t nq = 0, k = 0;
    SearchPlan plan{};             // route, k', bound, nq_pad, N of this search (search_plan.h)
    uint64_t* out_ids = nullptr;
    float* out_scores = nullptr;
    // Each slot has its own stream and its own workspaces, so the tail of search s (compaction,
    // re-score, certificate, read-back) can run beside the head -- and, on the stream path, the
    // scan -- of search s+1.  Only the corpus (read-only during a search) is shared.
    hipStream_t stream = nullptr;
    DevMem<uint32_t> flags;        // [0] bad-value flag, [1] max query norm^2 bits, [2] max err bits, [64..] pacing counters, then claim bits (kSlotFlagBytes)
    DevBuf q_raw, q_lp, scores, keys_a, keys_b, lists, small, hist, cand_rows, cand_fast, cand_canon;
    DevBuf q_f32;                  // prepared queries (the exact path re-reads them)
    DevBuf dump;                   // MFMA path: spill regions of the 4-wave kernel's hit logs (scratch, mfma_dump_bytes)
    DevBuf q_planes;               // split pass: [nq_pad][3 * ldp] bf16, [hi_j | lo_j | hi_j] per K-tile j
    // band pass (second chance of the queries whose certificate failed, search_complete)
    DevBuf band_idx, band_q, band_q_lp, band_planes, band_small, band_ids, band_scores;
    uint32_t pace_launches = 0;    // scan launches of this search so far (pacing-counter regions)
    uint32_t* h_readback = nullptr;   // pinned host block: status[nq] + 4 scalars, one D2H per search
    size_t h_readback_words = 0;
    hipEvent_t done = nullptr;     // recorded behind the D2H
    hipEvent_t scans_done = nullptr;   // recorded behind the last scan launch
    hipEvent_t mid_done = nullptr;     // recorded behind the second-to-last scan launch of a staged MFMA search (else with scans_done)
    bool mid_recorded = false;         // ... in the search being enqueued
    std::vector<hipEvent_t> ev;    // profiling events
    size_t ev_used = 0, t0 = 0, t1 = 0;
    std::vector<std::pair<size_t, size_t>> scan_pairs;
    int sample_pair = -1;          // index in scan_pairs of the sample-pass launch (-1: none)
    int tail_pair = -1;            // index in scan_pairs of the last filtered launch of a staged MFMA search: timed by idx->tail_ev[seq & 3]
    uint32_t seq = 0;              // number of this search on its handle (n_begun when it was enqueued)
    bool early_sample = false;     // its sample pass was ordered in front of the previous search's last stage
    uint32_t kp_boost_used = 1;    // the candidate-margin multiplier this search was enqueued with
    vrod_search_stats st{};
    // a synchronous search that times its own launches starts from no event in use
    void reset_events() { ev_used = 0; scan_pairs.clear(); sample_pair = -1; tail_pair = -1; }

    // hipGraph replay of small, launch-bound searches (search_enqueue): the launches of a search
    // whose every pointer and size equals the captured one are replayed as one graph launch
    struct GraphKey {
        const void *q = nullptr, *oi = nullptr, *os = nullptr, *corpus = nullptr, *xn = nullptr, *mask = nullptr;
        const void* bufs[12] = {};
        uint64_t N = 0, id_offset = 0;
        uint32_t nq = 0, k = 0;
        int path = 0;
        bool operator==(const GraphKey& o) const { return memcmp(this, &o, sizeof *this) == 0; }
    };
    GraphKey gkey{};               // of the last search enqueued in this slot
    bool gkey_valid = false;
    hipGraphExec_t gexec = nullptr;   // captured for gkey_graph
    GraphKey gkey_graph{};
    bool graph_off = false;        // a capture failed once: this slot stays on plain launches
    // what a replay must restore of the enqueue's host-side results
    SearchPlan g_plan{};
    vrod_search_stats g_st{};
};

// ------------------------------------------------------------------ the index
struct vrod_index {
    int device = 0;
    int num_cus = 256;
    uint32_t dim = 0, ld = 0;
    int dtype = VROD_DTYPE_F32, metric = VROD_METRIC_COSINE;
    size_t esize = 4;
    uint64_t count = 0, capacity = 0, id_offset = 0;
    DevMem<> corpus;            // [capacity][ld]
    DevMem<float> xnorm2;       // [capacity]
    uint32_t* max_xn2_bits = nullptr;  // device scalar: max squared row norm (float bits), a word of `flags`
    hipStream_t stream = nullptr;
    int path = VROD_PATH_AUTO;
    int profiling = 0;
    vrod_search_stats stats{};

    // fp32 corpus: bf16 planes [hi | lo] of the prepared rows for the batched fast pass on the bf16
    // matrix cores (kernels_prep.hip split_rows_kernel), a second copy of the corpus.  Built lazily
    // for rows [0, planes_rows) at the next batched search, on by default while the device keeps a
    // margin of free memory beside them (VROD_F32_SPLIT=0: never, =1: always try).
    bool split_enabled = false;
    bool split_forced = false;     // VROD_F32_SPLIT=1: no memory-margin check, never switched off by the failure count
    uint32_t split_bad = 0;        // split searches that sent more than 1/8 of their queries to the exact path
    DevMem<> planes;               // [planes_cap][2 * ldp] bf16, [hi_j | lo_j] per 64-element K-tile j
    uint64_t planes_cap = 0, planes_rows = 0;
    uint32_t ldp = 0;              // dim rounded up to 64 (bf16 128-B lines)

    // deleted rows (vrod_index_delete): one bit per row of the capacity, bit r % 32 of word r / 32 set = row r deleted.
    // The host mirror is the truth; the device copy is allocated at the first delete and the kernels see it only
    // while some row is deleted (row_mask()), so a handle that never deleted runs exactly the launches it ran before.
    std::vector<uint32_t> del_bits;    // [capacity / 32]
    DevMem<uint32_t> del_dev;          // [capacity / 32] on the device, or empty
    uint64_t n_deleted = 0;
    uint64_t mask_gen = 0;             // bumped by every change of the row mask's contents (delete, set_filter)
    struct SampleWindow { uint64_t S = 0, N = 0, gen = 0, first = 0; bool valid = false; } sample_win;

    // allow-list filter (vrod_index_set_filter): the allowed rows (bit set = allowed) and the EFFECTIVE mask the kernels
    // get while a filter is set, deleted | ~allowed -- host mirrors over the capacity plus a device copy.  Rows past the
    // filter's n_rows (rows added later included) are not allowed: the effective mask grows with ones.
    bool filter_on = false;
    std::vector<uint32_t> allow_bits, eff_bits;   // [capacity / 32] while filter_on
    DevMem<uint32_t> eff_dev;                     // [capacity / 32] on the device while filter_on
    uint64_t n_eligible = 0;                      // rows < count that are live and allowed
    // gather path: ascending local indices of the eligible rows, built for mask generation list_gen
    DevBuf list_dev;
    uint64_t list_gen = UINT64_MAX, list_n = 0;

    // The row columns (RowColumn above; for_each_column below the struct is where a new one is registered).
    // row labels (vrod_index_set_labels): a labelled search on a handle that never set one treats every row as label 0.
    // No other search reads them.
    RowColumn<uint32_t> labels{0u, "labels", SNAP_LABELS};
    // A labelled search's dense groups run the ordinary search flow over ONE label's rows: while mask_ovr is set it
    // stands for row_mask() and elig_ovr for eligible().  Null outside vrod_search_labeled, so no other call path
    // changes what it launches.  The override has no host mirror and no generation: what is cached per mask_gen (sample
    // window, gather list, graphs) is bypassed under it, never refreshed.
    const uint32_t* mask_ovr = nullptr;
    uint64_t elig_ovr = 0;
    // row tags (vrod_index_set_tags): one 64-bit mask per row.  Only vrod_search_tagged and vrod_search_where read them.
    RowColumn<uint64_t> tags{0ull, "tags", SNAP_TAGS};
    // row values (vrod_index_set_values): one signed 64-bit value per row.  Only vrod_search_where reads them.
    RowColumn<int64_t> values{0ll, "values", SNAP_VALUES};
    // row keys (vrod_index_set_keys): one caller-chosen 64-bit key per row, VROD_ID_NONE until set, unique among the live
    // rows.  The device table (keys_plan.h, kernels_keys.hip) finds a key's row; it exists from the first set_keys on.
    // No search reads either.
    RowColumn<uint64_t> keys{kKeyNone, "keys", SNAP_KEYS};
    DevMem<uint64_t> ktab_keys;        // the table's two device arrays ...
    DevMem<uint32_t> ktab_rows;
    KeyTable ktab{};                   // ... as the kernels take them: a view, filled by keys_table_clear
    uint64_t key_occupied = 0;         // slots in use, stale ones included: at most ktab.slots / 2
    uint64_t keyed_live = 0;           // live rows whose key is not VROD_ID_NONE
    uint64_t key_rebuilds = 0, key_max_probe = 0;   // vrod_index_key_stats
    // Workspaces the synchronous searches share, one per role (DESIGN.md "Shared workspaces"): the handle is idle before
    // and after each of those calls, so no two of them hold one at once.
    //   host_q, host_args: a host form's raw queries or vectors, and its other arguments, on the device;
    //   list_ids / list_scores: the first-stage lists a search flow writes and one launch reads.  Two sets: vrod_knn_graph
    //     keeps two batches in flight and batch s uses set s & 1 (byid_plan.h); every other call takes set 0;
    //   out_col [nq][k] words (a grouped or multi-vector search's labels, a diversified search's selection values) and
    //     out_found [nq]: the result columns beside out_ids / out_scores, for a host form or a caller that passes none.
    DevBuf host_q, host_args, list_ids[2], list_scores[2], out_col, out_found;
    // labelled search workspaces: [table | totals | segment offsets], the per-block counts, the row lists, the per-slot
    // arrays, the work table, a dense group's mask / raw queries (its results go to the shared lists).  A tagged
    // search, which is synchronous too, uses the same buffers for the same things (its table holds predicates).
    DevBuf lab_tab, lab_cnt, lab_lists, lab_slots, lab_entries, lab_mask, lab_q;
    // ordered selection (vrod_index_select_ordered): the {key, id} records the sort works on, and the small block
    // [the select's histograms | its state | the collect pass's per-group counts].  The hit bitmap and the groups' hit
    // counts are lab_mask and lab_cnt, as for every row-predicate pass.
    DevBuf ord_rec, ord_ws;
    // row aggregation (vrod_index_aggregate_where): the global hash table with its counters in front (aggregate_plan.h
    // agg_table_view; at most 2^21 + 1 slots of 48 bytes), and the occupied slots as dense records for the host to order.
    DevBuf agg_tab, agg_out;
    // group centroids (vrod_index_centroids_where): the small block [max word | ordered keys | counts | the table slots'
    // ranks] (centroid_plan.h centroid_ws_view) and the accumulators [groups][dim] int64.  The groups and their table are
    // agg_tab / agg_out, the hit bitmap lab_mask, a host form's dense vectors raw_stage.
    DevBuf cen_ws, cen_acc;
    // grouped search workspaces (vrod_search_grouped): the per-query words [found | valid | the lists' queries] and the
    // dense stage's masks [<= 8][capacity / 32]
    DevBuf grp_small, grp_mask;
    // multi-vector search (vrod_search_multivec).  The document index: doc_rank[row] = the rank of the row's label among
    // the handle's distinct labels, ascending (doc_labels [n_docs]), built on the host from labels.host at the first search
    // that needs it and kept until set_labels, add or compact change what it was built from (update and delete do not);
    // a handle without labels is one document, label 0, and has no rank array.  Then the workspaces: the prepared vectors
    // of the whole call, the de-duplication's entry labels / tables / candidate labels, the per-query words, the dense
    // route's best [<= 8][n_docs] / S rows / absent bitmap, the candidate route's M per score slot and its pair arrays.
    DevBuf doc_rank, doc_labels;
    uint64_t n_docs = 0;
    bool doc_valid = false;
    DevBuf mv_q, mv_ent, mv_tab, mv_cand, mv_small, mv_best, mv_S, mv_absent, mv_M, mv_pairs;
    vrod_multivec_stats mv_stats{};
    // Searches whose queries are stored rows (vrod_search_by_ids, vrod_knn_graph, and the range scans of
    // vrod_index_find_near_duplicates) hand the search flow rows that are prepared already: while prep_ovr is not negative
    // it stands for prep_form(metric) in the launch that prepares a search's or a range scan's queries -- M_L2, the
    // take-as-given form of L2 and IP handles: nothing is normalised, and rounding a bf16 value to bf16 is the identity.
    // Everything else that launch sets up is unchanged.  Negative outside those entry points; a search under it is never
    // captured into a graph nor matched with a captured one.
    int prep_ovr = -1;
    // a graph's workspaces, one set per batch in flight as its lists: the lists without self [rows][k], and the batch's
    // [live rows | place of every row among them]
    DevBuf byid_out_ids[2], byid_out_scores[2], byid_map[2];
    // candidate-list searches (vrod_search_candidates, vrod_score_candidates): the lists' entries as local rows and the
    // per-query words [lengths | the queries by sort class, or the score launch's tile offsets].  The resolved segments go
    // to lab_lists, the slot tables to lab_slots: the segmented driver finds them where a labelled search leaves its own.
    DevBuf cand_rows, cand_small;

    // workspaces
    DevBuf raw_stage, out_ids, out_scores;
    // vrod_index_save: the two dense chunks the pack kernel writes and the copies to the host read (a handle made by
    // vrod_index_load used it the other way round)
    DevBuf snap_stage;
    // vrod_index_update: a chunk's prepared rows and their destination rows; vrod_index_compact: live rows below each
    // 32-row word (compact_plan.h compact_word_bases), and the xnorm2 entries of a staged chunk's rows
    DevBuf upd_stage, upd_dst, compact_ws, compact_xn2;
    // add / update / upsert from device memory: the list of a chunk's source rows (RowSource::pick) on the device
    DevBuf ingest_pick;
    // range searches (vrod_range_search): the pool of qualifying rows and its sort partner, and the small block
    // [total (u64) | the caller's thresholds [nq] | per-query counters [nq]]
    DevBuf range_pool, range_pool_b, range_small;
    DevMem<uint32_t> flags;     // [0] bad-value flag of the insert path; [8] max squared row norm
    Pending slot[2];
    // start / stop of the last filtered scan launch of the four most recent searches (Timer::arm_tail): the next search's
    // sample launch may overlap it, and measures by how much when it completes
    struct TailEv { hipEvent_t start = nullptr, stop = nullptr; bool armed = false; };
    TailEv tail_ev[4];
    // Self-tuning candidate margin of the batched scan: k' = k + margin * kp_boost.boost (search_plan.h choose_kp,
    // kp_boost_step; stepped by search_complete)
    KpBoost kp_boost{};
    uint32_t n_begun = 0, n_ended = 0;   // searches enqueued / completed: slot = counter & 1
    hipEvent_t caller_ev = nullptr;      // orders the caller's stream before ours

    uint32_t n_pending() const { return n_begun - n_ended; }

    // --- composite handle (vrod_index_create with n_devices > 1): the rows are dealt to the
    // shards in blocks of kShardBlock rows (global row r -> shard (r / B) % G, local row
    // (r / (B*G)) * B + r % B), every shard is a complete single-device index of its own, and a
    // search runs on all of them at once, then gathers and merges on the first device.
    std::vector<vrod_index*> shards;
    IdMap deal{};                        // a shard of a composite handle: how its local rows become global ids
    // One group per DISTINCT device of the handle: the shards living on it, an exchange stream, the
    // device's rank in the handle's RCCL communicator, and per pipeline slot the packed block this
    // device contributes ([M][block]: one list per local shard, "no result" lists up to M = the
    // largest group) and what it receives ([U][M][block]: every device's contribution).
    struct DevGroup {
        int device = 0;
        std::vector<size_t> members;     // indices into shards
        hipStream_t xstream = nullptr;
        ncclComm_t comm = nullptr;
        DevBuf send[2], recv[2];
        size_t filled_nk[2] = {0, 0};    // nq*k the unused list slots of send[] were last filled for (+1)
    };
    std::vector<DevGroup> groups;
    std::vector<std::pair<size_t, size_t>> shard_home;   // shard -> (group, position in the group)
    bool use_rccl = false;
    std::vector<DevBuf> sh_q[2];         // per slot, per shard: the batch's raw queries on the shard's device
    struct CompPending {
        uint32_t nq = 0, k = 0;
        uint64_t* out_ids = nullptr;     // device pointers on groups[0].device
        float* out_scores = nullptr;
        hipEvent_t caller_ev = nullptr;  // the caller's stream at _begin: the merge writes out_ids / out_scores behind it
        bool ordered = false;            // ... recorded for this search (device outputs)
    } cslot[2];
    bool composite() const { return !shards.empty(); }

    size_t row_bytes() const { return (size_t)ld * esize; }
    uint64_t live() const { return count - n_deleted; }
    // rows a search may return: live, and allowed while a filter is set
    uint64_t eligible() const { return mask_ovr ? elig_ovr : filter_on ? n_eligible : live(); }
    // what the kernels get as their row mask: the effective mask while a filter is set, else the deleted rows, and null
    // while nothing is deleted
    const uint32_t* row_mask() const { return mask_ovr ? mask_ovr : filter_on ? eff_dev.p : n_deleted ? del_dev.p : nullptr; }
    // its host mirror (meaningful while row_mask() is non-null)
    const std::vector<uint32_t>& mask_bits() const { return filter_on ? eff_bits : del_bits; }
};

static int set_device(const vrod_index* idx) {
    HIP_TRY(hipSetDevice(idx->device));
    return VROD_OK;
}

// Set `c` of the shared first-stage lists, grown for n entries.
static int grow_lists(vrod_index* idx, int c, size_t n) {
    VROD_TRY(idx->list_ids[c].ensure(n * 8));
    VROD_TRY(idx->list_scores[c].ensure(n * 4));
    return VROD_OK;
}

// ids a search of this index reports: row + id_offset, or the dealing map of a composite handle's shard
static IdMap idmap_of(const vrod_index* idx) {
    IdMap m = idx->deal;
    if (!m.block_rows) m.offset = idx->id_offset;
    return m;
}

static bool valid_metric(int metric) {
    return metric == VROD_METRIC_COSINE || metric == VROD_METRIC_L2 || metric == VROD_METRIC_IP;
}

// f(column, i) for every row column of the handle, i = 0 .. kRowColumns - 1, in the order of their snapshot sections.
// THE place to register a new column: growth, compaction, save and load reach the columns through here.
constexpr int kRowColumns = 4;
template <typename F>
static void for_each_column(vrod_index* idx, F&& f) {
    f(idx->labels, 0);
    f(idx->tags, 1);
    f(idx->values, 2);
    f(idx->keys, 3);
}

static void drop_planes(vrod_index* idx) {   // (rebuilt lazily)
    idx->planes.release();
    idx->planes_cap = idx->planes_rows = 0;
}

// Two phases.  The first builds every new block in a local and fills it on the handle's stream; whatever fails there
// returns with the handle untouched, and the locals give their memory back.  The second swaps the blocks in and cannot
// fail; the locals then hold the old blocks, which go when they do -- behind the drain, and after everything new exists.
static int index_reserve(vrod_index* idx, uint64_t n_rows) {
    const uint64_t want = round_up(std::max<uint64_t>(n_rows, 1), kRowTile);
    if (want <= idx->capacity) return VROD_OK;
    if (want > 0xFFFFFF00ull) return fail(VROD_ERR_UNSUPPORTED, "more than 2^32-256 rows per shard");
    hipStream_t s = idx->stream;
    const uint64_t count = idx->count;
    const size_t rb = idx->row_bytes(), used = count * rb, words = want / 32;
    DevMem<> nc, ncol[kRowColumns];
    DevMem<float> nx;
    DevMem<uint32_t> nd, ne;
    std::vector<uint32_t> eff_grown;
    HIP_TRY(nc.alloc(want * rb));
    hipError_t e = nx.alloc(want * sizeof(float));
    if (e != hipSuccess) return fail(VROD_ERR_OUT_OF_MEMORY, "hipMalloc norms: %s", hipGetErrorString(e));
    const char* what = "corpus";   // zero rows and zero norms past the count
    if (count) {
        e = hipMemcpyAsync(nc.p, idx->corpus.p, used, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nx.p, idx->xnorm2.p, count * sizeof(float), hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipMemsetAsync(nc.get<char>() + used, 0, want * rb - used, s);
    if (e == hipSuccess) e = hipMemsetAsync(nx.p + count, 0, (want - count) * sizeof(float), s);
    if (e == hipSuccess && idx->del_dev.p) {   // the deleted-row bitmap follows the capacity (once it exists)
        what = "deleted-row bitmap";
        e = nd.alloc(words * 4);
        if (e == hipSuccess) e = hipMemsetAsync(nd.p, 0, words * 4, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nd.p, idx->del_bits.data(), idx->del_bits.size() * 4, hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess && idx->filter_on) {   // the effective mask of a filter: the new rows are not allowed (ones)
        what = "filter's row mask";
        eff_grown = idx->eff_bits;
        eff_grown.resize(words, ~0u);
        e = ne.alloc(words * 4);
        if (e == hipSuccess) e = hipMemcpyAsync(ne.p, eff_grown.data(), words * 4, hipMemcpyHostToDevice, s);
    }
    for_each_column(idx, [&](auto& c, int i) {   // the columns that exist: the new rows carry their default
        if (e == hipSuccess) { what = c.noun; e = c.stage_grow(count, want, s, ncol[i]); }
    });
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);   // (nothing is still aimed at a block that goes)
        return fail(VROD_ERR_HIP, "growing the %s failed: %s", what, hipGetErrorString(e));
    }

    // ---- from here on nothing fails
    idx->corpus.swap(nc);
    idx->xnorm2.swap(nx);
    for_each_column(idx, [&](auto& c, int i) { c.commit_grow(want, ncol[i]); });
    drop_planes(idx);
    if (idx->del_dev.p) idx->del_dev.swap(nd);
    idx->del_bits.resize(words, 0u);
    if (idx->filter_on) {
        idx->eff_dev.swap(ne);
        idx->eff_bits.swap(eff_grown);
        idx->allow_bits.resize(words, 0u);
    }
    idx->capacity = want;
    return VROD_OK;
}

// Word `w` of idx->flags.p as the launches on `s` so far leave it; a raised word is cleared for the next call.
static int take_flag(vrod_index* idx, uint32_t w, hipStream_t s, uint32_t* bad) {
    *bad = 0;
    HIP_TRY(hipMemcpyAsync(bad, &idx->flags.p[w], 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (*bad) {
        HIP_TRY(hipMemsetAsync(&idx->flags.p[w], 0, 4, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return VROD_OK;
}

static int check_bad_flag(vrod_index* idx, const char* what) {
    uint32_t bad;
    VROD_TRY(take_flag(idx, 0, idx->stream, &bad));
    if (bad) return fail(VROD_ERR_INVALID_VALUE, "%s contain NaN or Inf", what);
    return VROD_OK;
}

// ------------------------------------------------------------------ the rows of an add / update / upsert (ingest_plan.h RowSource)
// VROD_INGEST_STAGE=1: every device source goes the way of one on another device (packed, copied peer to peer, ingested
// from the dense copy), so that a one-GPU box can rehearse that way.  Read per call.
static bool ingest_force_stage() {
    const char* e = getenv("VROD_INGEST_STAGE");
    return e && e[0] == '1';
}

// Rows [0, m) of `src` become prepared rows [m][ld] at `out` (on idx's device, which is current), on idx->stream; NaN /
// Inf raise idx->flags.p[0].  One staging step says where the kernel finds them: host rows are uploaded to raw_stage (a
// picked list of them gathered first), a synthetic chunk is generated there, device rows on this GPU are read where they
// lie, device rows on another GPU (or all of them under VROD_INGEST_STAGE=1) are packed there and copied over.  raw_stage may still feed the previous chunk's
// launch: whatever fills it does so in the order of idx->stream, or drains that stream first.
static int ingest_prepare(vrod_index* idx, const RowSource& src, uint64_t m, void* out) {
    const uint32_t dim = idx->dim;
    const bool in_place = src.kind == RowSource::DEVICE && src.device == idx->device && !ingest_force_stage();
    const size_t bytes = (size_t)m * dim * ingest_elem_bytes(src.dtype);   // of the chunk, dense
    if (!in_place) VROD_TRY(idx->raw_stage.ensure(bytes));
    const void* p = idx->raw_stage.p;
    uint64_t stride = dim;
    const uint64_t* d_pick = nullptr;
    if (src.kind == RowSource::HOST) {
        if (src.pick) {   // one upload of the chunk's rows, gathered; the buffer goes with this step, so the copy is waited for
            std::unique_ptr<float[]> rows(new float[(size_t)m * dim]);
            rows_gather(src, dim, m, rows.get());
            HIP_TRY(hipMemcpyAsync(idx->raw_stage.p, rows.get(), bytes, hipMemcpyHostToDevice, idx->stream));
            HIP_TRY(hipStreamSynchronize(idx->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(idx->raw_stage.p, src.p, bytes, hipMemcpyHostToDevice, idx->stream));
        }
    } else if (src.kind == RowSource::SYNTH) {
        for (uint64_t i = 0; i < m;) {
            const uint64_t run = src.pick ? pick_run(src.pick, m, i) : m;
            launch_synth_rows(src.seed, src.first_row + (src.pick ? src.pick[i] : 0), run, dim, idx->raw_stage.as<float>() + i * dim, idx->stream);
            i += run;
        }
    } else if (in_place) {
        if (src.pick) {
            VROD_TRY(idx->ingest_pick.ensure(m * 8));
            HIP_TRY(hipMemcpyAsync(idx->ingest_pick.p, src.pick, m * 8, hipMemcpyHostToDevice, idx->stream));
            d_pick = idx->ingest_pick.as<uint64_t>();
        }
        p = src.p;
        stride = src.stride;
    } else {   // pack the rows on their device (dense, in their own type), copy them peer to peer
        HIP_TRY(hipStreamSynchronize(idx->stream));
        HIP_TRY(hipSetDevice(src.device));
        int rc = VROD_OK;
        {
            DevBuf pack, picks;   // on the source's device, for this chunk only
            rc = pack.ensure(bytes);
            if (rc == VROD_OK && src.pick) rc = picks.ensure(m * 8);
            hipError_t e = hipSuccess;
            if (rc == VROD_OK && src.pick) e = hipMemcpy(picks.p, src.pick, m * 8, hipMemcpyHostToDevice);
            if (rc == VROD_OK && e == hipSuccess) {
                launch_ingest_pack(src.p, src.dtype, src.stride, src.pick ? picks.as<uint64_t>() : nullptr, m, dim, pack.p, nullptr);
                e = hipGetLastError();
            }
            if (rc == VROD_OK && e == hipSuccess) e = hipMemcpyPeerAsync(idx->raw_stage.p, idx->device, pack.p, src.device, bytes, nullptr);
            if (rc == VROD_OK && e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (rc == VROD_OK && e != hipSuccess) rc = fail(VROD_ERR_HIP, "staging rows from device %d: %s", src.device, hipGetErrorString(e));
        }
        HIP_TRY(hipSetDevice(idx->device));
        VROD_TRY(rc);
    }
    launch_ingest_rows(p, src.dtype, stride, d_pick, m, dim, idx->ld, prep_form(idx->metric), idx->dtype, &idx->flags.p[0], out, idx->stream);
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}

static int index_add(vrod_index* idx, const RowSource& src, uint64_t n) {
    if (!n) return VROD_OK;
    VROD_TRY(set_device(idx));
    idx->doc_valid = false;   // (the document index of a multi-vector search covers the rows it was built from)
    if (idx->count + n > idx->capacity) {
        uint64_t want = std::max(idx->count + n, idx->capacity + idx->capacity / 2);
        if (src.kind == RowSource::SYNTH || idx->capacity == 0) want = idx->count + n;
        VROD_TRY(index_reserve(idx, want));
    }
    const uint64_t count0 = idx->count;
    // the max squared row norm is accumulated (atomicMax) by the very launches whose rows may be
    // rejected: keep the value it had, so that a rejected add cannot widen (or, with an Inf row,
    // void) the certificate bound of every later search
    HIP_TRY(hipMemcpyAsync(&idx->flags.p[9], idx->max_xn2_bits, 4, hipMemcpyDeviceToDevice, idx->stream));
    const uint64_t chunk = ingest_chunk_rows(n, idx->dim);
    for (uint64_t done = 0; done < n; done += chunk) {
        const uint64_t m = std::min(chunk, n - done);
        char* dst = (char*)idx->corpus.p + idx->count * idx->row_bytes();
        VROD_TRY(ingest_prepare(idx, rows_from(src, done), m, dst));
        launch_row_fastnorm(dst, idx->dtype, m, idx->ld, idx->xnorm2.p + idx->count, idx->max_xn2_bits, idx->stream);
        HIP_TRY(hipGetLastError());
        idx->count += m;
    }
    int rc = check_bad_flag(idx, "rows");
    if (rc != VROD_OK) {  // roll back: re-zero the rows just written
        idx->count = count0;
        (void)hipMemsetAsync((char*)idx->corpus.p + count0 * idx->row_bytes(), 0, n * idx->row_bytes(), idx->stream);
        (void)hipMemsetAsync(idx->xnorm2.p + count0, 0, n * sizeof(float), idx->stream);
        (void)hipMemcpyAsync(idx->max_xn2_bits, &idx->flags.p[9], 4, hipMemcpyDeviceToDevice, idx->stream);
        (void)hipStreamSynchronize(idx->stream);
        return rc;
    }
    return VROD_OK;
}

// ------------------------------------------------------------------ update in place (vrod_index_update)
// One pass over the n rows of an update, in the chunks of index_add: each is prepared into upd_stage.
//   dst == null: prepare only.  The NaN / Inf check of a call that needs more than one chunk, and of every shard of a
//                composite handle: every row is checked before any row is written.  Returns what the flag says.
//   dst != null: row i goes to corpus row dst[i] (kScatterSkip: nowhere), with its xnorm2 entry, the running maximum
//                and its bf16 planes where they exist (kernels_mutate.hip).  check_first: the call fits one chunk and
//                has not been checked: the flag is read between the prepare and the scatter.
// Nothing but the scatter writes to the corpus, xnorm2 or max_xn2_bits, so a rejected update changes none of them.
static int index_update_pass(vrod_index* idx, const uint32_t* dst, const RowSource& src, uint64_t n, bool check_first) {
    VROD_TRY(set_device(idx));
    const uint64_t chunk = ingest_chunk_rows(n, idx->dim);
    VROD_TRY(idx->upd_stage.ensure(chunk * idx->row_bytes()));
    if (dst) VROD_TRY(idx->upd_dst.ensure(chunk * 4));
    for (uint64_t done = 0; done < n; done += chunk) {
        const uint64_t m = std::min(chunk, n - done);
        VROD_TRY(ingest_prepare(idx, rows_from(src, done), m, idx->upd_stage.p));
        if (!dst) continue;
        if (check_first) VROD_TRY(check_bad_flag(idx, "rows"));
        HIP_TRY(hipMemcpyAsync(idx->upd_dst.p, dst + done, m * 4, hipMemcpyHostToDevice, idx->stream));
        launch_scatter_rows(idx->upd_stage.p, idx->upd_dst.as<uint32_t>(), m, idx->dtype, idx->ld, idx->corpus.p, idx->xnorm2.p, idx->max_xn2_bits,
                            idx->dtype == VROD_DTYPE_F32 ? idx->planes.p : nullptr, idx->planes_rows, idx->ldp, idx->stream);
        HIP_TRY(hipGetLastError());
    }
    if (!dst) return check_bad_flag(idx, "rows");
    HIP_TRY(hipStreamSynchronize(idx->stream));
    return VROD_OK;
}

// dst: per row of the call its local row, or kScatterSkip for an id that the call names again later
static int index_update(vrod_index* idx, const std::vector<uint32_t>& dst, const RowSource& src, uint64_t n) {
    if (n <= ingest_chunk_rows(n, idx->dim)) return index_update_pass(idx, dst.data(), src, n, true);
    VROD_TRY(index_update_pass(idx, nullptr, src, n, false));
    return index_update_pass(idx, dst.data(), src, n, false);
}

static void mask_changed(vrod_index* idx);

// ------------------------------------------------------------------ the key table (keys_plan.h, kernels_keys.hip)
constexpr uint32_t kKeyCtrWord = 64;   // idx->flags.p[64 .. 70): the table's device counters (KeyCounters)
static KeyCounters* key_ctr(const vrod_index* idx) { return (KeyCounters*)(idx->flags.p + kKeyCtrWord); }

// What the launches on the handle's stream left in the counters (the stream is drained).  `what` names the caller.
static int keys_take_counters(vrod_index* idx, const char* what, KeyCounters& c) {
    HIP_TRY(hipMemcpyAsync(&c, key_ctr(idx), sizeof c, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    if (c.err & kKeyErrFull)
        return fail(VROD_ERR_INTERNAL, "%s: a walk of the key table met no empty slot in %llu (%llu occupied)", what,
                    (unsigned long long)idx->ktab.slots, (unsigned long long)idx->key_occupied);
    return VROD_OK;
}

// An empty table sized for n keys (key_table_slots: it grows, never shrinks).  The old arrays go only when the new
// ones exist, so a caller that runs this before it writes anything has every allocation of a rebuild behind it.
static int keys_table_clear(vrod_index* idx, uint64_t n) {
    VROD_TRY(set_device(idx));
    const uint64_t slots = key_table_slots(n, idx->ktab.slots);
    if (slots != idx->ktab.slots) {
        DevMem<uint64_t> nk;
        DevMem<uint32_t> nr;
        HIP_TRY(nk.alloc(slots * 8));
        const hipError_t e = nr.alloc(slots * 4);
        if (e != hipSuccess) return fail(VROD_ERR_OUT_OF_MEMORY, "hipMalloc of the key table: %s", hipGetErrorString(e));
        idx->ktab_keys.swap(nk);   // (the old arrays go with the locals)
        idx->ktab_rows.swap(nr);
        idx->ktab.slot_key = idx->ktab_keys.p; idx->ktab.slot_row = idx->ktab_rows.p; idx->ktab.slots = slots;
    }
    HIP_TRY(hipMemsetAsync(idx->ktab.slot_key, 0xFF, slots * 8, idx->stream));
    HIP_TRY(hipMemsetAsync(idx->ktab.slot_row, 0, slots * 4, idx->stream));
    idx->key_occupied = 0;
    idx->key_max_probe = 0;
    return VROD_OK;
}
// The table anew from the live keyed rows of the key column as it stands, sized for n keys.  counted: it is a rebuild
// of vrod_key_stats (the first table of a handle, and a loaded handle's, are not).  *dup (may be null): two live rows
// hold one key -- with a null dup that is an internal error.
static int keys_rebuild(vrod_index* idx, uint64_t n, bool counted, const char* what, bool* dup = nullptr) {
    VROD_TRY(keys_table_clear(idx, n));
    hipStream_t s = idx->stream;
    HIP_TRY(hipMemsetAsync(key_ctr(idx), 0, sizeof(KeyCounters), s));
    launch_keys_insert(idx->ktab, idx->keys.d(), idx->del_dev.p, 0, idx->count, true, key_ctr(idx), s);
    HIP_TRY(hipGetLastError());
    KeyCounters c{};
    VROD_TRY(keys_take_counters(idx, what, c));
    idx->key_occupied = c.claimed;
    idx->key_max_probe = c.max_probe;
    if (counted) idx->key_rebuilds++;
    if (dup) *dup = (c.err & kKeyErrHeld) != 0;
    else if (c.err & kKeyErrHeld) return fail(VROD_ERR_INTERNAL, "%s: two live rows hold one key", what);
    return VROD_OK;
}

// The keys that rows [r0, r0 + n) of the key column hold go into the table (the load rule was seen to before).
static int keys_insert(vrod_index* idx, uint64_t r0, uint64_t n, const char* what) {
    hipStream_t s = idx->stream;
    HIP_TRY(hipMemsetAsync(key_ctr(idx), 0, sizeof(KeyCounters), s));
    launch_keys_insert(idx->ktab, idx->keys.d(), idx->del_dev.p, r0, n, false, key_ctr(idx), s);
    HIP_TRY(hipGetLastError());
    KeyCounters c{};
    VROD_TRY(keys_take_counters(idx, what, c));
    idx->key_occupied += c.claimed;
    idx->key_max_probe = std::max<uint64_t>(idx->key_max_probe, c.max_probe);
    return VROD_OK;
}

// ------------------------------------------------------------------ compaction (vrod_index_compact)
// The live rows move down in place, chunk by chunk on the handle's stream (compact_plan.h says why that is safe), with
// their xnorm2 entries; the vacated tail is zeroed again (the scan kernels rely on zero rows past the count), the maximum
// squared norm is taken afresh over the survivors (= a fresh handle's), the tombstones are cleared and a filter's allowed
// bits follow their rows.  The bf16 planes of an fp32 handle are not moved: planes_rows = 0 has the next batched search
// split the compacted rows again, which gives the bits a fresh handle's planes hold.
// Everything that can fail comes before the first row moves; a HIP error after that leaves the handle unusable.
static int index_compact(vrod_index* idx, uint64_t* out_new_ids) {
    idx->doc_valid = false;   // (rows move, labels may vanish: the document index is rebuilt by the next multi-vector search)
    const uint64_t count = idx->count;
    if (!idx->n_deleted) {
        if (out_new_ids) compact_new_ids(idx->del_bits.data(), count, idx->id_offset, out_new_ids);   // the identity
        return VROD_OK;
    }
    VROD_TRY(set_device(idx));
    const uint32_t* del = idx->del_bits.data();
    const size_t words = (size_t)((count + 31) / 32), cap_words = idx->del_bits.size();
    const size_t rb = idx->row_bytes();
    const uint64_t chunk_rows = std::max<uint64_t>(32, std::min<uint64_t>(kCompactChunkRows, (256ull << 20) / rb) / 32 * 32);
    const CompactPlan plan = plan_compact(del, count, chunk_rows);
    std::vector<uint32_t> base(words);
    compact_word_bases(del, count, base.data());
    std::vector<uint32_t> new_allow, new_eff;
    if (idx->filter_on) {
        new_allow.resize(cap_words);
        new_eff.resize(cap_words);
        compact_bits(del, idx->allow_bits.data(), count, new_allow.data(), cap_words);
        for (size_t w = 0; w < cap_words; ++w) new_eff[w] = ~new_allow[w];   // nothing is deleted afterwards
    }
    ColumnBytes moved[kRowColumns];   // the columns move with their rows; the vacated tail carries the default again
    for_each_column(idx, [&](auto& c, int i) { c.stage_compact(del, count, moved[i]); });
    uint64_t stage_rows = 0;
    for (const CompactChunk& c : plan.chunks) if (c.staged) stage_rows = std::max(stage_rows, c.L);
    if (stage_rows) {
        VROD_TRY(idx->raw_stage.ensure(stage_rows * rb));
        VROD_TRY(idx->compact_xn2.ensure(stage_rows * sizeof(float)));
    }
    VROD_TRY(idx->compact_ws.ensure(words * 4));
    HIP_TRY(hipMemcpyAsync(idx->compact_ws.p, base.data(), words * 4, hipMemcpyHostToDevice, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));

    // ---- from here on rows move
    hipStream_t s = idx->stream;
    char* corpus = (char*)idx->corpus.p;
    hipError_t e = hipSuccess;
    for (const CompactChunk& c : plan.chunks) {
        if (c.staged) {
            launch_compact_rows(corpus, idx->xnorm2.p, idx->del_dev.p, idx->compact_ws.as<uint32_t>(), c.r0, c.r1, rb, idx->raw_stage.p,
                                idx->compact_xn2.as<float>(), c.w0, s);
            e = hipMemcpyAsync(corpus + c.w0 * rb, idx->raw_stage.p, c.L * rb, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(idx->xnorm2.p + c.w0, idx->compact_xn2.p, c.L * sizeof(float), hipMemcpyDeviceToDevice, s);
        } else {
            launch_compact_rows(corpus, idx->xnorm2.p, idx->del_dev.p, idx->compact_ws.as<uint32_t>(), c.r0, c.r1, rb, corpus, idx->xnorm2.p, 0, s);
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) break;
    }
    if (e == hipSuccess) e = hipMemsetAsync(corpus + plan.live * rb, 0, (count - plan.live) * rb, s);
    if (e == hipSuccess) e = hipMemsetAsync(idx->xnorm2.p + plan.live, 0, (count - plan.live) * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(idx->max_xn2_bits, 0, 4, s);
    if (e == hipSuccess) { launch_xn2_max(idx->xnorm2.p, plan.live, idx->max_xn2_bits, s); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemsetAsync(idx->del_dev.p, 0, cap_words * 4, s);
    if (e == hipSuccess && idx->filter_on) e = hipMemcpyAsync(idx->eff_dev.p, new_eff.data(), cap_words * 4, hipMemcpyHostToDevice, s);
    for_each_column(idx, [&](auto& c, int i) { if (e == hipSuccess) e = c.upload_compact(moved[i], s); });
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess)
        return fail(VROD_ERR_HIP, "vrod_index_compact: %s while rows were moving: the handle is unusable, destroy it", hipGetErrorString(e));

    if (out_new_ids) compact_new_ids(del, count, idx->id_offset, out_new_ids);
    std::fill(idx->del_bits.begin(), idx->del_bits.end(), 0u);
    idx->n_deleted = 0;
    idx->count = plan.live;
    if (idx->filter_on) { idx->allow_bits.swap(new_allow); idx->eff_bits.swap(new_eff); }   // n_eligible: the same rows
    for_each_column(idx, [&](auto& c, int i) { c.commit_compact(moved[i]); });
    idx->planes_rows = 0;
    mask_changed(idx);
    if (idx->keys.exists()) VROD_TRY(keys_rebuild(idx, idx->keyed_live, true, "vrod_index_compact"));   // every slot named an old row
    return VROD_OK;
}

// ------------------------------------------------------------------ experiment switches
namespace vrod {
const DebugEnv& debug_env() {
    static const DebugEnv env = [] {
        DebugEnv d;
        auto num = [](const char* name, long long dflt) { const char* e = getenv(name); return e && *e ? atoll(e) : dflt; };
        auto on = [](const char* name) { const char* e = getenv(name); return !e || e[0] != '0'; };
        d.pace_kt = (int)num("VROD_DEBUG_PACE_KT", d.pace_kt);
        d.pace_tiles = (int)num("VROD_DEBUG_PACE", d.pace_tiles);
        d.w4_steal = on("VROD_DEBUG_W4_STEAL");
        d.skinny = on("VROD_DEBUG_SKINNY");
        d.stage_growth = (uint64_t)num("VROD_DEBUG_STAGE_GROWTH", 0);
        d.sample_rows = (uint64_t)num("VROD_DEBUG_SAMPLE_ROWS", 0);
        d.kp_margin = (uint32_t)num("VROD_DEBUG_KP_MARGIN", 0);
        if (const char* e = getenv("VROD_DEBUG_EARLY_SAMPLE")) d.early_sample = e[0] != '0' ? 1 : 0;
        d.sample_grouped = on("VROD_DEBUG_SAMPLE_GROUPED");
        d.graph = on("VROD_DEBUG_GRAPH");
        d.band = on("VROD_DEBUG_BAND");
        return d;
    }();
    return env;
}
}  // namespace vrod

// ------------------------------------------------------------------ search pipeline
struct Timer {
    vrod_index* idx;
    Pending& P;
    Timer(vrod_index* i, Pending& p) : idx(i), P(p) {}
    size_t mark() {
        if (idx->profiling < 2) return 0;   // stream markers only at level 2 (total_ms)
        if (P.ev_used == P.ev.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return 0;
            P.ev.push_back(e);
        }
        (void)hipEventRecord(P.ev[P.ev_used], P.stream);
        return P.ev_used++;
    }
    // two fresh events for the next scan launch (attached to the dispatch, not recorded as markers)
    void arm(size_t& a, size_t& b) {
        a = b = 0;
        if (!idx->profiling) return;
        while (P.ev.size() < P.ev_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return;
            P.ev.push_back(e);
        }
        a = P.ev_used++;
        b = P.ev_used++;
        g_launch_events.start = P.ev[a];
        g_launch_events.stop = P.ev[b];
    }
    float ms(size_t a, size_t b) {
        float m = 0.f;
        if (idx->profiling && a < P.ev_used && b < P.ev_used) (void)hipEventElapsedTime(&m, P.ev[a], P.ev[b]);
        return m;
    }
    // Markers around ONE launch on the slot's stream, for launches that take no launch-attached events: begin_launch in
    // front of it, end_launch behind it.  Nothing is created or recorded while profiling is off.
    int begin_launch(size_t& a, size_t& b) {
        a = b = 0;
        if (!idx->profiling) return VROD_OK;
        arm(a, b);
        g_launch_events = LaunchEvents{};
        if (b) HIP_TRY(hipEventRecord(P.ev[a], P.stream));
        return VROD_OK;
    }
    int end_launch(size_t a, size_t b) {
        if (idx->profiling && b) { HIP_TRY(hipEventRecord(P.ev[b], P.stream)); P.scan_pairs.push_back({a, b}); }
        return VROD_OK;
    }
    // the time between the markers of every launch so far, added to st.scan_ms (the stream is drained)
    void add_scan_ms(vrod_search_stats& st) {
        if (idx->profiling)
            for (size_t i = 0; i < P.scan_pairs.size(); ++i) st.scan_ms += ms(P.scan_pairs[i].first, P.scan_pairs[i].second);
    }
    // The LAST filtered launch of a staged MFMA search is timed by events of the handle's ring instead (tail_ev[seq & 3]):
    // the next search's sample pass may run beside it, and that search wants both intervals when it is completed --
    // by then this slot's own events belong to the search after it.
    void arm_tail() {
        if (!idx->profiling) return;
        vrod_index::TailEv& T = idx->tail_ev[P.seq & 3];
        if (!T.start && hipEventCreate(&T.start) != hipSuccess) return;
        if (!T.stop && hipEventCreate(&T.stop) != hipSuccess) return;
        g_launch_events.start = T.start;
        g_launch_events.stop = T.stop;
        T.armed = true;
        P.tail_pair = (int)P.scan_pairs.size();
    }
    float pair_ms(size_t i) {
        if ((int)i == P.tail_pair) {
            const vrod_index::TailEv& T = idx->tail_ev[P.seq & 3];
            float m = 0.f;
            if (idx->profiling && T.armed) (void)hipEventElapsedTime(&m, T.start, T.stop);
            return m;
        }
        return ms(P.scan_pairs[i].first, P.scan_pairs[i].second);
    }
    // ms during which this search's sample launch and the previous search's last filtered launch were BOTH in flight
    float sample_overlap_ms() {
        if (!idx->profiling || P.sample_pair < 0 || !P.early_sample || P.seq == 0) return 0.f;
        const vrod_index::TailEv& T = idx->tail_ev[(P.seq - 1) & 3];
        const size_t a = P.scan_pairs[P.sample_pair].first, b = P.scan_pairs[P.sample_pair].second;
        if (!T.armed || a >= P.ev_used || b >= P.ev_used) return 0.f;
        float tail_len = 0.f, s0 = 0.f, s1 = 0.f;   // everything relative to the start of that launch
        if (hipEventElapsedTime(&tail_len, T.start, T.stop) != hipSuccess) return 0.f;
        if (hipEventElapsedTime(&s0, T.start, P.ev[a]) != hipSuccess) return 0.f;
        if (hipEventElapsedTime(&s1, T.start, P.ev[b]) != hipSuccess) return 0.f;
        return std::max(0.f, std::min(s1, tail_len) - std::max(s0, 0.f));
    }
};

// select chain over fast (or canonical) scores of `nq` queries -> keys of <= kSelectChunk per query
// returns pointer/ld/n of the final key set through out params.
// (the handle's deleted rows are left out at the first level: they never reach the keys)
// `mask`: the row mask of the columns (the handle's row_mask() when column = row; null for the gather path's columns)
// `len` (a labelled search's segments): per query the number of its columns, n the largest of them
static int select_chain(vrod_index* idx, Pending& P, const float* d_scores, uint64_t score_ld, uint64_t n, int nq,
                        uint32_t kp, const uint32_t* mask, const uint64_t** out_keys, uint64_t* out_ld, uint64_t* out_n,
                        const uint32_t* len = nullptr) {
    const uint64_t nch0 = (n + kSelectChunk - 1) / kSelectChunk;
    const uint64_t ld_a = nch0 * kp;
    VROD_TRY(P.keys_a.ensure((size_t)nq * ld_a * 8));
    uint64_t cur_n = launch_select_from_scores(d_scores, score_ld, n, nq, score_form(idx->metric), kp, P.keys_a.as<uint64_t>(), ld_a,
                                               mask, P.stream, len);
    const uint64_t* cur = P.keys_a.as<uint64_t>();
    uint64_t cur_ld = ld_a;
    bool a_is_cur = true;
    while (cur_n > kSelectChunk) {
        const uint64_t nch = (cur_n + kSelectChunk - 1) / kSelectChunk;
        const uint64_t nld = nch * kp;
        DevBuf& dst = a_is_cur ? P.keys_b : P.keys_a;
        VROD_TRY(dst.ensure((size_t)nq * nld * 8));
        cur_n = launch_select_from_keys(cur, cur_ld, cur_n, nq, kp, dst.as<uint64_t>(), nld, P.stream);
        cur = dst.as<uint64_t>();
        cur_ld = nld;
        a_is_cur = !a_is_cur;
    }
    *out_keys = cur;
    *out_ld = cur_ld;
    *out_n = cur_n;
    return VROD_OK;
}

// ------------------------------------------------------------------ workspace layout of a slot
// P.small: [nq_pad] words each of fast query norms^2 | T (bound on the fast score of what a query left out) | thresholds
// | status, then the read-back block [nq + 4]
struct SmallBlock { float* qn2; float* T; float* thr; uint32_t* status; uint32_t* readback; };
static size_t small_bytes(uint32_t nq_pad) { return (size_t)nq_pad * 4 * 5 + 64; }
static SmallBlock small_block(const Pending& P) {
    const size_t n = P.plan.nq_pad;
    float* f = P.small.as<float>();
    uint32_t* status = (uint32_t*)(f + 3 * n);
    return {f, f + n, f + 2 * n, status, status + n};
}
// P.lists (MFMA path): [nq_pad][kSelectChunk] hit lists {score bits, row}, the per-query counters behind them
struct ListBlock { uint2* lists; uint32_t* counts; };
static size_t list_bytes(uint32_t nq_pad) { return (size_t)nq_pad * kSelectChunk * 8 + (size_t)nq_pad * 4; }
static ListBlock list_block(const Pending& P) {
    return {P.lists.as<uint2>(), (uint32_t*)((char*)P.lists.p + (size_t)P.plan.nq_pad * kSelectChunk * 8)};
}
// the slot's pacing-counter and claim-bit regions of scan launch `launch` (kSlotFlagBytes: behind the 64 scalars)
static uint32_t* pace_region(const Pending& P, uint32_t launch) { return P.flags.p + 64 + (launch % kPaceRegions) * kPaceWords; }
static uint32_t* claim_region(const Pending& P, uint32_t launch) {
    return P.flags.p + 64 + kPaceRegions * kPaceWords + (launch % kPaceRegions) * kClaimWords;
}
static const size_t kHistWords = 8 * 4096 + 8;   // stream path: [8][<=4096] bin counters + 8 key counters

// ------------------------------------------------------------------ MFMA launches
// Scan arguments of a block of `nq` queries (`nq_pad` rows of `queries`) over the corpus, appending to the slot's list block
static int mfma_args(vrod_index* idx, Pending& P, MfmaScanArgs& a, const void* queries, const float* qn2, const float* thr,
                     uint32_t nq, uint32_t nq_pad) {
    const ListBlock L = list_block(P);
    a = MfmaScanArgs{};
    a.corpus = idx->corpus.p; a.queries = queries; a.xnorm2 = idx->xnorm2.p; a.qnorm2 = qn2; a.thr = thr;
    a.lists = L.lists; a.counts = L.counts; a.cap = kSelectChunk; a.ld = idx->ld; a.nq_pad = nq_pad; a.nq = nq;
    a.metric = score_form(idx->metric);
    a.row_mask = idx->row_mask();
    VROD_TRY(P.dump.ensure(mfma_dump_bytes(idx->num_cus)));
    a.dump = P.dump.p;
    return VROD_OK;
}

// Point `a` at the bf16 planes (SPLIT form of the kernels): the corpus's [hi_j | lo_j], and the [hi_j | lo_j | hi_j]
// planes of the block's queries, made here into `q_planes` from their `nq_pad` prepared fp32 rows.
static int use_split_planes(vrod_index* idx, MfmaScanArgs& a, const float* q_f32, uint32_t nq_pad, DevBuf& q_planes, hipStream_t s) {
    VROD_TRY(q_planes.ensure((size_t)nq_pad * 3 * idx->ldp * 2));
    launch_split_rows(q_f32, nq_pad, idx->ld, idx->ldp, q_planes.p, true, s);
    a.corpus = idx->planes.p; a.queries = q_planes.p;
    a.ld = 3 * idx->ldp;                          // K extent = query row
    a.lda_bytes = 2 * idx->ldp * 2;               // corpus row [hi_j | lo_j] per K-tile
    a.a_wrap = 1;                                 // SPLIT form of the kernel
    return VROD_OK;
}

// Filtered launches of `a` over rows [lo, end).  A launch addresses rows relative to its first tile with 24 bits: the
// range is cut at 2^24 rows.  Every launch takes the slot's next pacing / claim region (P.pace_launches); the search's
// own launches (`fresh`) find the first kPaceRegions of them zeroed by the query preparation, later ones -- and every
// launch of the band pass -- reuse a region behind a memset.  `tail`: the last launch is the search's last filtered
// launch (Timer::arm_tail).
static void launch_filtered(vrod_index* idx, Pending& P, Timer& tm, MfmaScanArgs& a, int scan_dtype, uint64_t lo, uint64_t end,
                            bool fresh, bool tail) {
    vrod_search_stats& st = P.st;
    const double row_bytes_alg = (double)idx->ld * idx->esize;
    while (lo < end) {
        const uint64_t e = std::min<uint64_t>(end, lo / kRowTile * kRowTile + (1ull << 24));
        a.row_begin = (uint32_t)lo; a.row_end = (uint32_t)e;
        a.pace = pace_region(P, P.pace_launches);
        a.pace_is_zero = fresh && P.pace_launches < kPaceRegions;
        a.claims = claim_region(P, P.pace_launches);
        a.claims_is_zero = a.pace_is_zero;
        ++P.pace_launches;
        size_t e0, e1;
        tm.arm(e0, e1);
        if (tail && e == end) tm.arm_tail();
        launch_scan_mfma(a, scan_dtype, idx->num_cus, P.stream);
        P.scan_pairs.push_back({e0, e1});
        st.scan_launches++;
        st.scan_bytes += (double)(e - lo / kRowTile * kRowTile) * row_bytes_alg;
        st.scan_flops += 2.0 * a.nq * (double)(e - lo) * idx->dim;
        lo = e;
    }
}

// The event behind a search's last scan launch; a search that did not mark an earlier point (mid_done: behind the
// second-to-last stage of a staged MFMA search) marks it here as well.
static int record_scans_done(Pending& P, hipStream_t s) {
    if (!P.mid_recorded) { HIP_TRY(hipEventRecord(P.mid_done, s)); P.mid_recorded = true; }
    HIP_TRY(hipEventRecord(P.scans_done, s));
    return VROD_OK;
}

static Pending& other_slot(vrod_index* idx, Pending& P) { return idx->slot[&P == &idx->slot[0] ? 1 : 0]; }

// The bf16 planes of an fp32 corpus are a second copy of it, allocated for the whole capacity: without room for them
// the handle switches the split pass off and quietly keeps the fp32 pass.
static bool planes_ready(vrod_index* idx) {
    if (idx->planes_cap >= idx->capacity) return true;
    drop_planes(idx);
    const size_t want = idx->capacity * 2ull * idx->ldp * 2ull;
    bool room = true;
    if (!idx->split_forced) {
        // by default the planes must leave the caller a margin: 1/8 of the device or 4 GiB
        size_t free_b = 0, total_b = 0;
        room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= want + std::max<size_t>(total_b / 8, (size_t)4 << 30);
    }
    if (room && idx->planes.alloc(want) == hipSuccess) {
        idx->planes_cap = idx->capacity;
        return true;
    }
    (void)hipGetLastError();
    idx->split_enabled = false;
    return false;
}

// -------- fast pass A: HBM-bound scan of <= 8 queries at a time, all N fast scores kept, radix select (pass 1 fused
// into the scan; its histogram block was cleared by the query preparation)
static int stream_pass(vrod_index* idx, Pending& P, Timer& tm, bool in_graph) {
    const uint64_t N = P.plan.N;
    const uint32_t nq = P.nq, kp = P.plan.kp;
    const int form = score_form(idx->metric);
    const SmallBlock B = small_block(P);
    vrod_search_stats& st = P.st;
    hipStream_t s = P.stream;
    const uint64_t score_ld = round_up(N, 64);
    VROD_TRY(P.scores.ensure((size_t)8 * score_ld * 4));
    VROD_TRY(P.keys_a.ensure((size_t)8 * kSelectChunk * 8));
    uint32_t* d_hist = P.hist.as<uint32_t>();
    uint32_t* d_cnt = d_hist + 8 * 4096;
    // one HBM-bound scan at a time (two would only share the bandwidth and stretch each
    // other); everything behind the scan overlaps the other slot's scan
    if (!in_graph) HIP_TRY(hipStreamWaitEvent(s, other_slot(idx, P).scans_done, 0));
    const double row_bytes_alg = (double)idx->ld * idx->esize;
    const uint32_t qpp = (uint32_t)stream_max_queries_per_pass(idx->ld);   // queries per pass: 8, fewer for long rows
    for (uint32_t q0 = 0; q0 < nq; q0 += qpp) {
        const int nqc = (int)std::min<uint32_t>(qpp, nq - q0);
        int nqp = 1;
        while (nqp < nqc) nqp <<= 1;
        if (q0 > 0) HIP_TRY(hipMemsetAsync(d_hist, 0, kHistWords * 4, s));
        size_t a, b;
        tm.arm(a, b);
        launch_scan_stream(idx->corpus.p, idx->dtype, form, idx->ld, N, P.q_f32.as<float>() + (size_t)q0 * idx->ld, nqp,
                           P.scores.as<float>(), score_ld, d_hist, kp, idx->row_mask(), s);
        P.scan_pairs.push_back({a, b});
        if (q0 + qpp >= nq && !in_graph) VROD_TRY(record_scans_done(P, s));
        st.scan_launches++;
        st.scan_bytes += (double)N * row_bytes_alg;
        st.scan_flops += 2.0 * nqc * (double)N * idx->dim;
        launch_hist_compact(P.scores.as<float>(), score_ld, N, nqc, form, d_hist, stream_hist_bits(nqp), kp,
                            P.keys_a.as<uint64_t>(), kSelectChunk, d_cnt, B.status + q0, idx->row_mask(), s);
        launch_keys_to_candidates(P.keys_a.as<uint64_t>(), kSelectChunk, kSelectChunk, nqc, form, kp,
                                  P.cand_rows.as<uint32_t>() + (size_t)q0 * kp, P.cand_fast.as<float>() + (size_t)q0 * kp,
                                  B.T + q0, d_cnt, s);
    }
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}

// First row of the sample pass's S rows on a handle with a row mask (deleted rows, or a filter: the window's rows that a
// search may not return).  Any window gives a valid threshold (its masked rows are masked to the worst score, and every
// window row is scanned again by the filtered stages), but one made of masked rows gives none: the first stage would
// then append every row, overflow its lists and send every query to the exact path.  The window stays at row 0 while
// at least 7/8 of it is eligible; else it moves to the tile-aligned window with the most eligible rows (first of
// equals).  Cached until the mask or the stage plan changes.
// (The rank j is taken among the window's eligible rows without rescaling: the first stage's rows are as sparse in
// eligible rows as the window's, so its expected hits per query stay ~j * (stage rows) / S whatever the filter's
// density -- only a window with fewer than j eligible rows loosens the threshold to the worst score, and then the
// first stage has about as few eligible rows to append.)
static uint64_t sample_window(vrod_index* idx, uint64_t S, uint64_t N) {
    if (!idx->row_mask() || S >= N) return 0;
    if (idx->mask_ovr) return 0;   // one label's mask (a labelled search): no host mirror to weigh windows by, nothing cached
    vrod_index::SampleWindow& W = idx->sample_win;
    if (W.valid && W.S == S && W.N == N && W.gen == idx->mask_gen) return W.first;
    const uint64_t tiles = N / kRowTile, wt = S / kRowTile;   // S < N is a whole number of tiles (plan_stages)
    const std::vector<uint32_t>& mb = idx->mask_bits();
    std::vector<uint32_t> live(tiles);
    for (uint64_t t = 0; t < tiles; ++t) {
        uint32_t dead = 0;
        for (uint32_t w = 0; w < kRowTile / 32; ++w) dead += (uint32_t)__builtin_popcount(mb[t * (kRowTile / 32) + w]);
        live[t] = kRowTile - dead;
    }
    uint64_t cur = 0;
    for (uint64_t t = 0; t < wt; ++t) cur += live[t];
    uint64_t best = cur, first = 0;
    if (cur * 8 < S * 7) {
        for (uint64_t t = 1; t + wt <= tiles; ++t) {
            cur += live[t + wt - 1];
            cur -= live[t - 1];
            if (cur > best) { best = cur; first = t * kRowTile; }
        }
    }
    W = {S, N, idx->mask_gen, first, true};
    return first;
}

// -------- gather path (VROD_PATH_GATHER): the canonical score of the eligible rows only, for every query of the batch,
// and an exact select by (score, id).  No fast pass, no certificate: exact by construction.
// The row list -- ascending local indices of the eligible rows -- is built on the host from the mask's mirror and
// uploaded once per mask generation.  The generation only changes while the handle is idle (delete and set_filter
// require it), and a completed search's launches are behind its done event: no launch still reads the old list.
static int gather_list(vrod_index* idx) {
    if (idx->list_gen == idx->mask_gen && idx->list_n == idx->eligible()) return VROD_OK;
    const uint32_t* mask = idx->row_mask() ? idx->mask_bits().data() : nullptr;
    std::vector<uint32_t> rows;
    rows.reserve(idx->eligible());
    for (uint64_t w = 0; w * 32 < idx->count; ++w) {
        uint32_t keep = mask ? ~mask[w] : ~0u;
        if (idx->count - w * 32 < 32) keep &= (1u << (idx->count - w * 32)) - 1u;
        while (keep) {
            rows.push_back((uint32_t)(w * 32 + (uint32_t)__builtin_ctz(keep)));
            keep &= keep - 1u;
        }
    }
    if (!rows.empty()) {
        VROD_TRY(idx->list_dev.ensure(rows.size() * 4));
        HIP_TRY(hipMemcpy(idx->list_dev.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    }
    idx->list_n = rows.size();
    idx->list_gen = idx->mask_gen;
    return VROD_OK;
}

static int gather_pass(vrod_index* idx, Pending& P, Timer& tm) {
    VROD_TRY(gather_list(idx));
    const uint64_t m = idx->list_n;
    const uint32_t nq = P.nq, k = P.k;
    const int form = score_form(idx->metric);
    vrod_search_stats& st = P.st;
    hipStream_t s = P.stream;
    const uint32_t* list = idx->list_dev.as<uint32_t>();
    // queries per launch: the whole batch while its score block [g][m] stays under 1 GiB (as the exact path's)
    const uint64_t score_ld = round_up(m, 64);
    uint64_t g = std::max<uint64_t>(1, (1ull << 30) / (score_ld * 4));
    if (g >= nq) g = nq;
    else if (g > 8) g = g / 8 * 8;
    const uint32_t kx = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, m), kSelectChunk / 2);   // (the rest: unfilled)
    VROD_TRY(P.scores.ensure((size_t)g * score_ld * 4));
    for (uint32_t q0 = 0; q0 < nq; q0 += (uint32_t)g) {
        const uint32_t gc = (uint32_t)std::min<uint64_t>(g, nq - q0);
        size_t a = 0, b = 0;
        if (idx->profiling) {   // (no launch-attached events here: markers around the launch)
            tm.arm(a, b);
            g_launch_events = LaunchEvents{};
            if (b) HIP_TRY(hipEventRecord(P.ev[a], s));
        }
        launch_rescore_list(idx->corpus.p, idx->dtype, form, idx->dim, idx->ld, P.q_f32.as<float>() + (size_t)q0 * idx->ld, gc, list, m,
                            P.scores.as<float>(), score_ld, s);
        if (idx->profiling && b) {
            HIP_TRY(hipEventRecord(P.ev[b], s));
            P.scan_pairs.push_back({a, b});
        }
        st.scan_launches++;
        const uint64_t* keys; uint64_t kld, kn;
        VROD_TRY(select_chain(idx, P, P.scores.as<float>(), score_ld, m, (int)gc, kx, nullptr, &keys, &kld, &kn));
        launch_list_keys_to_output(keys, kld, kn, (int)gc, form, k, list, idmap_of(idx), P.out_ids + (size_t)q0 * k,
                                   P.out_scores + (size_t)q0 * k, s);
    }
    VROD_TRY(record_scans_done(P, s));
    st.scan_bytes = (double)m * idx->ld * idx->esize;
    st.scan_flops = 2.0 * nq * (double)m * idx->dim;
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}

// -------- fast pass B: batched MFMA scan.  (1) dense sample pass over the first S rows, (2) exact j-th best per query =
// threshold, (3) filtered launches over the stages of plan_stages, (4) after each stage keep the best k' of every list.
static int mfma_pass(vrod_index* idx, Pending& P, Timer& tm, const void* q_lp) {
    const SearchPlan& plan = P.plan;
    const uint64_t N = plan.N;
    const uint32_t nq = P.nq, kp = plan.kp, cap = kSelectChunk;
    const int form = score_form(idx->metric);
    const SmallBlock B = small_block(P);
    const ListBlock L = list_block(P);
    vrod_search_stats& st = P.st;
    hipStream_t s = P.stream;
    // The MFMA scans own the whole chip.  Two orders of the two searches in flight:
    //  late : the sample pass behind the other slot's last scan, the first filtered stage behind its read-back --
    //         the other search's tail (compaction, re-score, certificate, read-back) and this one's sample + select
    //         side by side, ~95 us per batch in which nothing else runs (profiles/r02/s_pipeline_timeline_shard.txt);
    //  early: the sample pass + select (~50 us) in front of the other slot's LAST stage (behind its second-to-last:
    //         mid_done), the first filtered stage behind that last stage: it starts the moment the other search's
    //         scans are through and runs beside that search's tail.
    // Same box, batch 1024 x 768 bf16, early against late: 1.25M rows 1.84-1.85 / 1.87 ms, 2.5M 3.52 / 3.56-3.58,
    // 5M 6.76 / 6.83, 10M 13.28-13.32 / 13.40-13.41 (-1.4 / -1.5 / -1.0 / -0.7 %).  Early is taken up to 6M rows per
    // handle: beyond, the gain is under 1 % and the sample pass squeezed beside a 7-ms stage makes that stage's own
    // launch time (what bench.py's roofline divides by) unreadable.  VROD_DEBUG_EARLY_SAMPLE=0 / 1 forces late / early.
    const int early_env = debug_env().early_sample;
    const bool early = early_env >= 0 ? early_env == 1 : N <= 6000000ull;
    Pending& O = other_slot(idx, P);
    HIP_TRY(hipStreamWaitEvent(s, early ? O.mid_done : O.scans_done, 0));
    MfmaScanArgs a;
    VROD_TRY(mfma_args(idx, P, a, idx->dtype == VROD_DTYPE_BF16 ? q_lp : P.q_f32.p, B.qn2, B.thr, nq, plan.nq_pad));
    if (plan.split) {
        // planes of the rows added since the last batched search, and of this batch's queries
        if (idx->planes_rows < N) {
            launch_split_rows((const float*)idx->corpus.p + idx->planes_rows * idx->ld, N - idx->planes_rows, idx->ld, idx->ldp,
                              (char*)idx->planes.p + idx->planes_rows * 2ull * idx->ldp * 2ull, false, s);
            if (round_up(N, kRowTile) > N)   // the tile padding rows stay zero
                HIP_TRY(hipMemsetAsync((char*)idx->planes.p + N * 2ull * idx->ldp * 2ull, 0, (round_up(N, kRowTile) - N) * 2ull * idx->ldp * 2ull, s));
            idx->planes_rows = N;
        }
        VROD_TRY(use_split_planes(idx, a, P.q_f32.as<float>(), plan.nq_pad, P.q_planes, s));
    }
    const int scan_dtype = plan.split ? VROD_DTYPE_BF16 : idx->dtype;
    P.pace_launches = 0;
    std::vector<uint64_t> bounds{N};
    if (N > cap) {
        const uint32_t nqb = plan.nq_pad / 256;
        const StagePlan sp = plan_stages(N, kp, cap, std::max<uint32_t>(1, (uint32_t)idx->num_cus / nqb) * kRowTile,
                                         debug_env().stage_growth, debug_env().sample_rows);
        bounds = sp.bounds;
        MfmaScanArgs d = a;
        const uint64_t w0 = sample_window(idx, sp.S, N);
        d.row_begin = (uint32_t)w0; d.row_end = (uint32_t)(w0 + sp.S);
        // Grouped form where the kernel has it: the threshold is the j-th best of the per-group bests (groups of 32
        // rows: valid -- at least j rows are that good -- and exact unless two of the j best share a group), 1/32 of
        // the dense block to write and to select from.  Only while the groups outnumber j by 8x (else: every score).
        // A handle with deleted rows (or a filter) takes every score: a group's best may be a masked row, and at 10 %
        // masked rows nearly every group holds one.
        const bool group_env = debug_env().sample_grouped && !idx->row_mask();
        const uint32_t grows = group_env ? mfma_dense_group_rows(d, scan_dtype) : 0u;
        const uint32_t n_groups = grows ? (uint32_t)(round_up(sp.S, kRowTile) / grows) : 0u;
        const bool grouped = grows && (uint64_t)sp.j * 8 <= n_groups && sp.S % kRowTile == 0;   // whole tiles of real rows
        const uint32_t dense_ld = grouped ? (uint32_t)round_up(n_groups, 64) : (uint32_t)round_up(sp.S, kRowTile);
        const uint32_t n_sel = grouped ? n_groups : sp.S;
        VROD_TRY(P.scores.ensure((size_t)plan.nq_pad * dense_ld * 4));
        d.dense_out = P.scores.as<float>(); d.dense_ld = dense_ld; d.dense_grouped = grouped;
        d.pace = pace_region(P, P.pace_launches++); d.pace_is_zero = true;
        size_t e0, e1;
        tm.arm(e0, e1);
        launch_scan_mfma(d, scan_dtype, idx->num_cus, s);
        P.sample_pair = (int)P.scan_pairs.size();
        P.early_sample = early;
        P.scan_pairs.push_back({e0, e1});
        st.scan_launches++;
        // (the sample rows are scanned again by the first filtered stage: their time counts, their flops and
        // bytes do not -- algorithmic work is 2 * nq * N * d and N * row bytes, each row once)
        launch_mask_sample(P.scores.as<float>(), dense_ld, n_sel, (int)nq, w0, idx->row_mask(), form, s);   // (no mask: nothing)
        launch_sample_select(P.scores.as<float>(), dense_ld, n_sel, (int)nq, form, sp.j, B.thr, s);
    }
    HIP_TRY(hipStreamWaitEvent(s, early ? O.scans_done : O.done, 0));
    uint64_t lo = 0;
    for (size_t li = 0; li < bounds.size(); ++li) {
        const bool last = li + 1 == bounds.size();
        launch_filtered(idx, P, tm, a, scan_dtype, lo, bounds[li], true, last);
        lo = std::max(lo, bounds[li]);
        if (li + 2 == bounds.size()) { HIP_TRY(hipEventRecord(P.mid_done, s)); P.mid_recorded = true; }
        if (last) VROD_TRY(record_scans_done(P, s));
        launch_list_compact(L.lists, L.counts, cap, (int)nq, form, kp, B.thr, B.status, last ? P.cand_rows.as<uint32_t>() : nullptr,
                            last ? P.cand_fast.as<float>() : nullptr, last ? B.T : nullptr, s);
    }
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}

// Enqueue one search into slot P: every launch up to the D2H of the status block.  Returns
// without waiting for the device (except on the trivial empty-corpus case).
static int search_enqueue_body(vrod_index* idx, Pending& P, const float* d_queries_raw, uint32_t nq, uint32_t k,
                               uint64_t* d_out_ids, float* d_out_scores, bool in_graph) {
    vrod_search_stats& st = P.st;
    st = vrod_search_stats{};
    st.nq = nq;
    st.k = k;
    P.nq = nq; P.k = k; P.out_ids = d_out_ids; P.out_scores = d_out_scores;
    P.trivial = true;
    P.mid_recorded = false;
    P.ev_used = 0; P.t0 = P.t1 = 0; P.scan_pairs.clear(); P.sample_pair = -1;
    P.tail_pair = -1; P.early_sample = false; P.seq = idx->n_begun;
    idx->tail_ev[P.seq & 3].armed = false;
    if (!nq) return VROD_OK;
    hipStream_t s = P.stream;
    Timer tm(idx, P);
    P.t0 = tm.mark();

    // ---- plan (search_plan.h)
    const uint64_t N = idx->count;
    const int form = score_form(idx->metric);
    // the gather path: forced, or AUTO over a filter narrow enough (search_plan.h filter_route)
    const bool gather = !idx->mask_ovr && (idx->path == VROD_PATH_GATHER || (idx->filter_on && filter_route(idx->path, idx->dtype, N, idx->eligible(), nq, idx->dim)));
    Route r = gather ? Route{VROD_PATH_GATHER, false}
                     : route(idx->path, idx->dtype, idx->split_enabled, mfma_skinny_max_queries(true, 2u * idx->ldp * 2u), N, nq, k);
    if (r.split && !planes_ready(idx)) r.split = false;
    P.plan = make_plan(r.path, r.split, form, idx->dim, N, nq, k, idx->kp_boost.boost, debug_env().kp_margin);
    const SearchPlan& plan = P.plan;
    P.kp_boost_used = idx->kp_boost.boost;
    st.kprime = gather ? 0u : plan.kp;   // (the gather path re-scores every eligible row: no candidates)
    st.path = plan.path;
    st.split_pass = plan.split ? 1u : 0u;

    if (N == 0 || idx->eligible() == 0) {  // empty corpus, or no row deleted and allowed: every slot unfilled
        std::vector<uint64_t> hi((size_t)nq * k, UINT64_MAX);
        std::vector<uint32_t> hs((size_t)nq * k, kScoreNoneBits);
        HIP_TRY(hipMemcpyAsync(d_out_ids, hi.data(), hi.size() * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_out_scores, hs.data(), hs.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        return VROD_OK;
    }

    // ---- prepare queries (one launch): q_f32 [nq_pad][ld] fp32 (zero padded), q_lp bf16 copy,
    // fast norms, NaN/Inf flag, max |q|^2.  No host round trip: the certificate forms its bound
    // on the device and the flag is read with the results.
    const uint32_t nq_pad = plan.nq_pad;
    const bool mfma = plan.path == VROD_PATH_MFMA;
    P.trivial = false;
    if (!P.done) HIP_TRY(hipEventCreateWithFlags(&P.done, hipEventDisableTiming));
    VROD_TRY(P.q_f32.ensure((size_t)nq_pad * idx->ld * 4));
    void* q_lp = nullptr;
    if (idx->dtype == VROD_DTYPE_BF16) {
        VROD_TRY(P.q_lp.ensure((size_t)nq_pad * idx->ld * 2));
        q_lp = P.q_lp.p;
    }
    VROD_TRY(P.small.ensure(small_bytes(nq_pad)));
    if (P.h_readback_words < (size_t)nq + 4) {
        if (P.h_readback) (void)hipHostFree(P.h_readback);
        P.h_readback = nullptr;
        P.h_readback_words = 0;
        HIP_TRY(hipHostMalloc((void**)&P.h_readback, ((size_t)nq + 4 + 1024) * 4, hipHostMallocDefault));
        P.h_readback_words = (size_t)nq + 4 + 1024;
    }
    if (mfma) VROD_TRY(P.lists.ensure(list_bytes(nq_pad)));
    const SmallBlock B = small_block(P);
    // the MFMA path's per-query list counters / thresholds are reset by the same launch that prepares the queries
    // (padding queries get the BEST score as threshold so that they never append)
    const uint32_t worst_bits = form == M_COSINE ? 0xFF800000u : 0x7F800000u;  // -inf / +inf
    QueryInit qi{};
    qi.status = B.status;
    qi.counts = mfma ? list_block(P).counts : nullptr;
    qi.thr = mfma ? B.thr : nullptr;
    qi.thr_live_bits = worst_bits;
    qi.thr_pad_bits = worst_bits ^ 0x80000000u;
    // (flags[0..2] -- bad-value flag, max |q|^2 bits, max err bits -- are zero here: cleared by the
    // read-back launch of the slot's previous search, never by the launch that accumulates into them)
    qi.zero_words = nullptr;
    qi.n_zero_words = 0;
    // MFMA path: the pacing-counter and claim-bit regions of the first kPaceRegions scan launches (stream path: the
    // histogram block of the first pass of 8 queries) are zeroed by the launch that prepares the queries
    qi.zero_words2 = mfma ? pace_region(P, 0) : nullptr;
    qi.n_zero_words2 = kPaceRegions * (kPaceWords + kClaimWords);
    if (plan.path == VROD_PATH_STREAM) {
        VROD_TRY(P.hist.ensure(kHistWords * 4));
        qi.zero_words2 = P.hist.as<uint32_t>();
        qi.n_zero_words2 = (uint32_t)kHistWords;
    }
    launch_prep_queries(d_queries_raw, nq, nq_pad, idx->dim, idx->ld, idx->prep_ovr >= 0 ? idx->prep_ovr : prep_form(idx->metric), idx->dtype,
                        P.q_f32.as<float>(), q_lp, B.qn2, &P.flags.p[0], &P.flags.p[1], qi, s);
    HIP_TRY(hipGetLastError());

    // ---- fast pass: k' candidates per query + T
    VROD_TRY(P.cand_rows.ensure((size_t)nq * plan.kp * 4));
    VROD_TRY(P.cand_fast.ensure((size_t)nq * plan.kp * 4));
    VROD_TRY(P.cand_canon.ensure((size_t)nq * plan.kp * 4));
    if (plan.path == VROD_PATH_STREAM) VROD_TRY(stream_pass(idx, P, tm, in_graph));
    else if (mfma) VROD_TRY(mfma_pass(idx, P, tm, q_lp));
    else if (gather) VROD_TRY(gather_pass(idx, P, tm));

    if (plan.path != VROD_PATH_EXACT && !gather) {
        // -------- canonical re-score + final ordering + certificate
        launch_rescore_candidates(idx->corpus.p, idx->dtype, form, idx->dim, idx->ld, P.q_f32.as<float>(), (int)nq,
                                  P.cand_rows.as<uint32_t>(), plan.kp, P.cand_canon.as<float>(), s);
        launch_final_topk(P.cand_rows.as<uint32_t>(), P.cand_fast.as<float>(), P.cand_canon.as<float>(), B.T, (int)nq, plan.kp, k,
                          form, idmap_of(idx), plan.eps_mode, plan.eps_c, &P.flags.p[1], idx->max_xn2_bits, d_out_ids, d_out_scores,
                          B.status, (float*)&P.flags.p[2], s);
    }
    launch_gather_readback(B.status, nq, P.flags.p, idx->max_xn2_bits, B.readback, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(P.h_readback, B.readback, ((size_t)nq + 4) * 4, hipMemcpyDeviceToHost, s));
    P.t1 = tm.mark();
    if (!in_graph) HIP_TRY(hipEventRecord(P.done, s));
    return VROD_OK;
}

// Small searches are launch-bound (10k x 128, one query: ~9 launches, 80 us, of which the kernels
// are a fraction): when a slot sees the same search again -- same query / output pointers, sizes,
// corpus and workspaces -- its launches are captured into a hipGraph on the third occurrence and
// replayed as ONE graph launch from then on.  Only the stream path with a single scan pass over a
// small corpus and with profiling off qualifies; anything else, and any capture failure, takes the
// plain launches.
static int search_enqueue(vrod_index* idx, Pending& P, const float* d_queries_raw, uint32_t nq, uint32_t k,
                          uint64_t* d_out_ids, float* d_out_scores) {
    const bool graphs_on = debug_env().graph;
    const uint64_t N = idx->count;
    // (measured at 10k x 128, one query: a replay costs the HOST less -- 50 vs 65 us per search with two
    // in flight -- but is no faster end to end than plain launches, 91 vs 82 us synchronous: only
    // searches begun while another one is pending, i.e. host-bound pipelines, take it)
    // (a gather search is never replayed: the filter route decides before graph_route)
    const bool gather = !idx->mask_ovr && (idx->path == VROD_PATH_GATHER || (idx->filter_on && filter_route(idx->path, idx->dtype, N, idx->eligible(), nq, idx->dim)));
    // (nor a search whose queries are stored rows: the captured launch prepares its queries, theirs are prepared)
    const bool graphable = graphs_on && idx->prep_ovr < 0 && !P.graph_off && idx->profiling == 0 && nq >= 1 && nq <= 8 && idx->eligible() > 0 && idx->n_pending() >= 1 &&
                           !gather && graph_route(idx->path, nq) && (double)N * idx->ld * idx->esize <= 64.0 * 1048576.0;
    Pending::GraphKey key{};
    if (graphable) {
        key.q = d_queries_raw; key.oi = d_out_ids; key.os = d_out_scores; key.corpus = idx->corpus.p; key.xn = idx->xnorm2.p;
        key.mask = idx->row_mask();
        const void* bufs[12] = {P.q_f32.p, P.q_lp.p, P.small.p, P.hist.p, P.scores.p, P.keys_a.p, P.cand_rows.p, P.cand_fast.p,
                                P.cand_canon.p, P.h_readback, P.flags.p, idx->max_xn2_bits};
        memcpy(key.bufs, bufs, sizeof bufs);
        key.N = N; key.id_offset = idmap_of(idx).offset; key.nq = nq; key.k = k; key.path = idx->path;
    }
    Pending& O = other_slot(idx, P);
    hipStream_t s = P.stream;
    if (graphable && P.gexec && P.gkey_graph == key) {
        // ---- replay
        P.st = P.g_st;
        P.nq = nq; P.k = k; P.out_ids = d_out_ids; P.out_scores = d_out_scores;
        P.trivial = false; P.ev_used = 0; P.t0 = P.t1 = 0; P.scan_pairs.clear();
        P.plan = P.g_plan;
        HIP_TRY(hipStreamWaitEvent(s, O.scans_done, 0));
        HIP_TRY(hipGraphLaunch(P.gexec, s));
        P.mid_recorded = false;
        VROD_TRY(record_scans_done(P, s));
        HIP_TRY(hipEventRecord(P.done, s));
        return VROD_OK;
    }
    const bool capture = graphable && P.gkey_valid && P.gkey == key;   // seen before with these very buffers
    if (capture) {
        if (P.gexec) { (void)hipGraphExecDestroy(P.gexec); P.gexec = nullptr; }
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            int rc = search_enqueue_body(idx, P, d_queries_raw, nq, k, d_out_ids, d_out_scores, true);
            hipGraph_t g = nullptr;
            const hipError_t e1 = hipStreamEndCapture(s, &g);
            hipError_t e2 = hipErrorUnknown;
            if (rc == VROD_OK && e1 == hipSuccess && g) e2 = hipGraphInstantiate(&P.gexec, g, nullptr, nullptr, 0);
            if (g) (void)hipGraphDestroy(g);
            if (rc == VROD_OK && e1 == hipSuccess && e2 == hipSuccess) {
                P.gkey_graph = key;
                P.g_plan = P.plan; P.g_st = P.st;
                HIP_TRY(hipStreamWaitEvent(s, O.scans_done, 0));
                HIP_TRY(hipGraphLaunch(P.gexec, s));
                VROD_TRY(record_scans_done(P, s));
                HIP_TRY(hipEventRecord(P.done, s));
                return VROD_OK;
            }
            (void)hipGetLastError();
            if (P.gexec) { (void)hipGraphExecDestroy(P.gexec); P.gexec = nullptr; }
        } else {
            (void)hipGetLastError();
        }
        P.graph_off = true;   // nothing was launched: fall through to the plain launches
    }
    const int rc = search_enqueue_body(idx, P, d_queries_raw, nq, k, d_out_ids, d_out_scores, false);
    if (graphable && rc == VROD_OK) {
        // the key is taken AFTER the body: its ensure() calls may have moved a workspace
        const void* bufs[12] = {P.q_f32.p, P.q_lp.p, P.small.p, P.hist.p, P.scores.p, P.keys_a.p, P.cand_rows.p, P.cand_fast.p,
                                P.cand_canon.p, P.h_readback, P.flags.p, idx->max_xn2_bits};
        memcpy(key.bufs, bufs, sizeof bufs);
        P.gkey = key;
        P.gkey_valid = true;
    } else {
        P.gkey_valid = false;
    }
    return rc;
}

// ------------------------------------------------------------------ band pass
// Second chance for the queries whose certificate failed on the MFMA path (exact duplicates and near-ties around
// the k-th result: real embedding corpora are full of them).  The exact path costs one pass over the corpus per 8
// queries; a batch where most queries fail would take seconds.  Instead ONE more filtered scan, shared by all failed
// queries, collects for each the rows whose fast score lies within the error bound of c_k, the k-th canonical
// score the first pass found (kernels_select.hip band_prepare_kernel: a superset of the true top-k, boundary ties
// included); their canonical re-score and an exact select by (score, id) is the answer -- no certificate needed.
// A query whose band holds more than kBandKeep rows (thousands of exact duplicates) stays on the exact path.
// (From how many failed queries on: kBandMinQueries*, search_plan.h band_eligible.)
static const uint32_t kBandKeep = kSelectChunk / 2;

static int band_pass(vrod_index* idx, Pending& P, std::vector<uint32_t>& failed, uint32_t max_qn2_bits) {
    const uint32_t nf = (uint32_t)failed.size(), k = P.k;
    const uint64_t N = P.plan.N;
    if (!debug_env().band || !band_eligible(P.plan, idx->dtype, nf, k)) return VROD_OK;
    vrod_search_stats& st = P.st;
    hipStream_t s = P.stream;
    Timer tm(idx, P);
    const uint32_t nf_pad = (uint32_t)round_up(nf, 256);
    const uint32_t cap = kSelectChunk;
    VROD_TRY(P.band_idx.ensure((size_t)nf_pad * 4));
    VROD_TRY(P.band_q.ensure((size_t)nf_pad * idx->ld * 4));
    void* bq_lp = nullptr;
    if (idx->dtype == VROD_DTYPE_BF16) {
        VROD_TRY(P.band_q_lp.ensure((size_t)nf_pad * idx->ld * 2));
        bq_lp = P.band_q_lp.p;
    }
    VROD_TRY(P.band_small.ensure((size_t)nf_pad * 4 * 5));   // thr | qn2 | ok | resolved | status (scratch)
    float* b_thr = P.band_small.as<float>();
    float* b_qn2 = b_thr + nf_pad;
    uint32_t* b_ok = (uint32_t*)(b_qn2 + nf_pad);
    uint32_t* b_res = b_ok + nf_pad;
    uint32_t* b_status = b_res + nf_pad;
    // the list block of the search is free again: its candidates were emitted
    const ListBlock L = list_block(P);
    HIP_TRY(hipMemcpyAsync(P.band_idx.p, failed.data(), (size_t)nf * 4, hipMemcpyHostToDevice, s));
    // the batch's max |q|^2 (the bound's norm): the device copy was consumed with the read-back, flags[3] holds it for this pass
    HIP_TRY(hipMemcpyAsync(&P.flags.p[3], &max_qn2_bits, 4, hipMemcpyHostToDevice, s));
    launch_gather_query_rows(P.q_f32.as<float>(), P.band_idx.as<uint32_t>(), nf, nf_pad, idx->ld, P.band_q.as<float>(), bq_lp, s);
    launch_band_prepare(P.band_idx.as<uint32_t>(), nf, nf_pad, P.out_scores, k, score_form(idx->metric), P.plan.eps_mode, P.plan.eps_c, &P.flags.p[3],
                        idx->max_xn2_bits, small_block(P).qn2, b_thr, b_qn2, L.counts, b_ok, s);
    MfmaScanArgs a;
    VROD_TRY(mfma_args(idx, P, a, idx->dtype == VROD_DTYPE_BF16 ? bq_lp : P.band_q.p, b_qn2, b_thr, nf, nf_pad));
    if (P.plan.split) VROD_TRY(use_split_planes(idx, a, P.band_q.as<float>(), nf_pad, P.band_planes, s));
    // (the pacing / claim regions were used by the search's own launches: never taken as zeroed)
    launch_filtered(idx, P, tm, a, P.plan.split ? VROD_DTYPE_BF16 : idx->dtype, 0, N, false, false);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> hcnt(nf), hok(nf);
    HIP_TRY(hipMemcpyAsync(hcnt.data(), L.counts, (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(hok.data(), b_ok, (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t need = (uint32_t)std::min<uint64_t>(k, idx->eligible());
    uint32_t maxc = 0, n_res = 0;
    std::vector<uint32_t> hres(nf_pad, 0u);
    for (uint32_t f = 0; f < nf; ++f) {
        // (a band shorter than k would mean the bound does not hold: never resolve on it)
        if (hok[f] && hcnt[f] >= need && hcnt[f] <= kBandKeep) { hres[f] = 1u; maxc = std::max(maxc, hcnt[f]); ++n_res; }
    }
    if (n_res) {
        uint32_t kpb = 32;
        while (kpb < maxc) kpb <<= 1;
        kpb = std::min<uint32_t>(std::max<uint32_t>(kpb, k), kBandKeep);
        VROD_TRY(P.cand_rows.ensure((size_t)nf * kpb * 4));
        VROD_TRY(P.cand_fast.ensure((size_t)nf * kpb * 4));
        VROD_TRY(P.cand_canon.ensure((size_t)nf * kpb * 4));
        VROD_TRY(P.band_ids.ensure((size_t)nf * k * 8));
        VROD_TRY(P.band_scores.ensure((size_t)nf * k * 4));
        HIP_TRY(hipMemcpyAsync(b_res, hres.data(), (size_t)nf_pad * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(b_status, 0, (size_t)nf_pad * 4, s));
        // every band row of a resolved query is kept (count <= kpb): sorted by fast score, padded with empty slots
        launch_list_compact(L.lists, L.counts, cap, (int)nf, score_form(idx->metric), kpb, b_thr, b_status, P.cand_rows.as<uint32_t>(), P.cand_fast.as<float>(),
                            b_qn2 /* T: unused */, s);
        launch_rescore_candidates(idx->corpus.p, idx->dtype, score_form(idx->metric), idx->dim, idx->ld, P.band_q.as<float>(), (int)nf, P.cand_rows.as<uint32_t>(), kpb,
                                  P.cand_canon.as<float>(), s);
        // flags[4]: the band's own observed |fast - canonical| (folded into max_fast_err by search_complete: the band is a
        // superset of the true top-k only while that stays inside the bound)
        HIP_TRY(hipMemsetAsync(&P.flags.p[4], 0, 4, s));
        launch_final_topk(P.cand_rows.as<uint32_t>(), P.cand_fast.as<float>(), P.cand_canon.as<float>(), b_qn2, (int)nf, kpb, k, score_form(idx->metric), idmap_of(idx),
                          P.plan.eps_mode, P.plan.eps_c, &P.flags.p[3], idx->max_xn2_bits, P.band_ids.as<uint64_t>(), P.band_scores.as<float>(), b_status,
                          (float*)&P.flags.p[4], s);
        launch_scatter_results(P.band_ids.as<uint64_t>(), P.band_scores.as<float>(), P.band_idx.as<uint32_t>(), b_res, nf, k, P.out_ids, P.out_scores, s);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> still;
        for (uint32_t f = 0; f < nf; ++f)
            if (!hres[f]) still.push_back(failed[f]);
        failed.swap(still);
        st.band_queries = n_res;
    }
    return VROD_OK;
}

// Complete the search in slot P: wait for its status block, then run the exact path for the
// queries whose certificate failed (enqueued behind whatever the stream holds by now).
static int search_complete(vrod_index* idx, Pending& P) {
    vrod_search_stats& st = P.st;
    hipStream_t s = P.stream;
    Timer tm(idx, P);
    const uint32_t nq = P.nq, k = P.k;
    const uint64_t N = P.plan.N;
    if (P.trivial) {
        idx->stats = st;
        return VROD_OK;
    }
    HIP_TRY(hipEventSynchronize(P.done));
    std::vector<uint32_t> hstatus(P.h_readback, P.h_readback + nq);
    uint32_t hflags[3];
    memcpy(hflags, P.h_readback + nq, 12);
    const uint32_t hmaxx = P.h_readback[nq + 3];
    if (P.plan.path == VROD_PATH_EXACT) {
        std::fill(hstatus.begin(), hstatus.end(), 1u);
    } else {
        memcpy(&st.max_fast_err, &hflags[2], 4);
        float qn2, xn2;
        memcpy(&qn2, &hflags[1], 4);
        memcpy(&xn2, &hmaxx, 4);
        st.eps_bound = eps_bound(P.plan.eps_mode, P.plan.eps_c, qn2, xn2);
    }
    if (hflags[0]) {  // NaN/Inf in the queries: whatever was computed is void (flag reset on device)
        idx->stats = st;
        return fail(VROD_ERR_INVALID_VALUE, "queries contain NaN or Inf");
    }

    // -------- exact path for uncertified queries: canonical score of every row, exact select.
    // Up to 8 queries share one pass over the corpus (their add chains are independent, so the
    // pass costs little more than one query's); the score block is kept under 1 GiB.
    std::vector<uint32_t> failed;
    for (uint32_t qi = 0; qi < nq; ++qi)
        if (hstatus[qi]) failed.push_back(qi);
    st.fallback_queries = (uint32_t)failed.size();
    if (!failed.empty()) VROD_TRY(band_pass(idx, P, failed, hflags[1]));   // resolves most of them with one more shared scan
    const bool many_failed = failed.size() * 8 > nq;   // what the band pass could not resolve (duplicates it handled cheaply do not count)
    if (P.plan.split && many_failed && !idx->split_forced && ++idx->split_bad >= 2) {
        // the split pass's bound is ~3x wider than the fp32 pass's: on a corpus whose gaps sit
        // inside it (twice now) the fp32 pass is the better fast pass.  The planes are released by
        // the next search that finds the handle idle.
        idx->split_enabled = false;
    }
    if (!failed.empty()) {
        const uint64_t score_ld = round_up(N, 64);
        int gmax = rescore_all_max_queries(idx->ld);
        while (gmax > 1 && (uint64_t)gmax * score_ld * 4 > (1ull << 30)) gmax >>= 1;
        const uint32_t kx = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, idx->eligible()), kSelectChunk / 2);   // (the rest: unfilled)
        for (size_t f0 = 0; f0 < failed.size();) {
            int g = gmax;
            while ((size_t)g > failed.size() - f0) g >>= 1;
            VROD_TRY(P.scores.ensure((size_t)g * score_ld * 4));
            launch_rescore_all(idx->corpus.p, idx->dtype, score_form(idx->metric), idx->dim, idx->ld, P.q_f32.as<float>(), &failed[f0], g, N,
                               P.scores.as<float>(), score_ld, s);
            const uint64_t* keys; uint64_t kld, kn;
            VROD_TRY(select_chain(idx, P, P.scores.as<float>(), score_ld, N, g, kx, idx->row_mask(), &keys, &kld, &kn));
            for (int i = 0; i < g; ++i) {
                const uint32_t qi = failed[f0 + i];
                launch_keys_to_output(keys + (size_t)i * kld, kn, score_form(idx->metric), k, idmap_of(idx), P.out_ids + (size_t)qi * k,
                                      P.out_scores + (size_t)qi * k, s);
            }
            HIP_TRY(hipGetLastError());
            f0 += g;
        }
    }
    if (st.fallback_queries) {
        P.t1 = tm.mark();
        HIP_TRY(hipStreamSynchronize(s));
        if (st.band_queries) {   // the band's re-score saw its own fast-vs-canonical differences
            float band_err = 0.f;
            HIP_TRY(hipMemcpy(&band_err, &P.flags.p[4], 4, hipMemcpyDeviceToHost));
            st.max_fast_err = std::max(st.max_fast_err, band_err);
        }
    }
    if (kp_boost_applies(P.plan, nq))   // the margin follows what the certificates say
        kp_boost_step(idx->kp_boost, P.kp_boost_used, st.fallback_queries != 0);
    if (idx->profiling) {
        for (size_t i = 0; i < P.scan_pairs.size(); ++i) st.scan_ms += tm.pair_ms(i);
        if (P.sample_pair >= 0 && (size_t)P.sample_pair < P.scan_pairs.size()) {
            st.sample_ms = tm.pair_ms((size_t)P.sample_pair);
            st.overlap_ms = tm.sample_overlap_ms();
        }
        if (idx->profiling >= 2) st.total_ms = tm.ms(P.t0, P.t1);
    }
    idx->stats = st;
    return VROD_OK;
}

// begin = take the next slot and enqueue; end = complete the oldest slot (FIFO).
static int search_begin(vrod_index* idx, const float* d_queries_raw, uint32_t nq, uint32_t k,
                        uint64_t* d_out_ids, float* d_out_scores) {
    if (idx->n_pending() >= 2) return fail(VROD_ERR_INVALID_ARG, "two searches are already pending: call vrod_search_end first");
    Pending& P = idx->slot[idx->n_begun & 1];
    if (idx->planes.p && !idx->split_enabled && idx->n_pending() == 0) drop_planes(idx);   // split pass switched off: give the planes back
    int rc = search_enqueue(idx, P, d_queries_raw, nq, k, d_out_ids, d_out_scores);
    if (rc != VROD_OK) {
        // a half-enqueued search: drain the stream, consume the per-search scalars, leave the slot free
        (void)hipStreamSynchronize(P.stream);
        (void)hipMemsetAsync(&P.flags.p[0], 0, 12, P.stream);
        (void)hipStreamSynchronize(P.stream);
        return rc;
    }
    P.active = true;
    idx->n_begun++;
    return VROD_OK;
}

static int search_end(vrod_index* idx) {
    if (idx->n_pending() == 0) return fail(VROD_ERR_INVALID_ARG, "no search is pending");
    Pending& P = idx->slot[idx->n_ended & 1];
    idx->n_ended++;
    P.active = false;
    return search_complete(idx, P);
}

// the slot (stream, raw-query buffer) the next search_begin will use
static Pending& next_slot(vrod_index* idx) { return idx->slot[idx->n_begun & 1]; }

static int run_search(vrod_index* idx, const float* d_queries_raw, uint32_t nq, uint32_t k,
                      uint64_t* d_out_ids, float* d_out_scores) {
    VROD_TRY(search_begin(idx, d_queries_raw, nq, k, d_out_ids, d_out_scores));
    return search_end(idx);
}

static int require_idle(const vrod_index* idx, const char* what) {
    if (idx->n_pending()) return fail(VROD_ERR_INVALID_ARG, "%s while a search is pending: call vrod_search_end first", what);
    return VROD_OK;
}

// The caller's stream holds the producers of the inputs and the last consumers of the output
// buffers: order it before ours without stopping the host.
static int order_after_caller(vrod_index* idx, void* stream) {
    if (!idx->caller_ev) HIP_TRY(hipEventCreateWithFlags(&idx->caller_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(idx->caller_ev, (hipStream_t)stream));
    HIP_TRY(hipStreamWaitEvent(next_slot(idx).stream, idx->caller_ev, 0));
    return VROD_OK;
}

// ------------------------------------------------------------------ composite (multi-device) handle
static const uint64_t kShardBlock = kDealBlock;   // (ingest_plan.h: the dealing is tested on the host there)

// global rows [first, first + n) cut at block boundaries: f(shard, global_first, count)
template <typename F>
static int for_each_piece(const vrod_index* idx, uint64_t first, uint64_t n, F&& f) {
    const uint64_t G = idx->shards.size();
    uint64_t r = first;
    const uint64_t end = first + n;
    while (r < end) {
        const uint64_t m = deal_piece_rows(r, end);
        VROD_TRY(f((size_t)deal_shard(r, G), r, m));
        r += m;
    }
    return VROD_OK;
}
static uint64_t local_row_of(const vrod_index* idx, uint64_t r) {
    return deal_local_row(r, idx->shards.size());
}

static int composite_add(vrod_index* idx, const RowSource& src, uint64_t n) {
    const uint64_t count0 = idx->count;
    for (vrod_index* sh : idx->shards) {   // what a roll-back restores (see index_add)
        VROD_TRY(set_device(sh));
        HIP_TRY(hipMemcpyAsync(&sh->flags.p[10], sh->max_xn2_bits, 4, hipMemcpyDeviceToDevice, sh->stream));
    }
    int rc = for_each_piece(idx, count0, n, [&](size_t g, uint64_t r, uint64_t m) {
        vrod_index* sh = idx->shards[g];
        if (sh->count != local_row_of(idx, r)) return fail(VROD_ERR_INTERNAL, "shard %zu is out of step", g);
        return index_add(sh, rows_from(src, r - count0), m);
    });
    if (rc != VROD_OK) {
        // a rejected piece (NaN/Inf) rolled itself back; drop the pieces already taken by other shards
        for (size_t g = 0; g < idx->shards.size(); ++g) {
            vrod_index* sh = idx->shards[g];
            uint64_t want = 0;   // local rows of shard g among global rows [0, count0)
            (void)for_each_piece(idx, 0, count0, [&](size_t gg, uint64_t, uint64_t m) { if (gg == g) want += m; return (int)VROD_OK; });
            if (sh->count > want) {
                (void)hipSetDevice(sh->device);
                (void)hipMemsetAsync((char*)sh->corpus.p + want * sh->row_bytes(), 0, (sh->count - want) * sh->row_bytes(), sh->stream);
                (void)hipMemsetAsync(sh->xnorm2.p + want, 0, (sh->count - want) * sizeof(float), sh->stream);
                sh->count = want;
            }
            (void)hipSetDevice(sh->device);
            (void)hipMemcpyAsync(sh->max_xn2_bits, &sh->flags.p[10], 4, hipMemcpyDeviceToDevice, sh->stream);
            (void)hipStreamSynchronize(sh->stream);
        }
        return rc;
    }
    idx->count = count0 + n;
    return VROD_OK;
}

// A change of the row mask's contents: the sample window and the gather list follow the generation, and a graph captured
// before holds the old mask (or the same pointer with other contents, or none): both slots drop theirs.
static void mask_changed(vrod_index* idx) {
    idx->mask_gen++;
    for (Pending& P : idx->slot) {
        if (P.gexec) { (void)hipGraphExecDestroy(P.gexec); P.gexec = nullptr; }
        P.gkey_valid = false;
    }
}

// "These rows are freshly dead", for every kind of delete (by id, by key, by predicate).  `fresh`: local rows (each <
// count) that were live until now, each once, whose bits the caller has set in the host mirror del_bits already, all
// within its words [wlo, whi].  The changed words go to the device (allocated for the whole capacity at the first
// delete), under a filter the effective mask follows, then the counts, the keys' live count and the mask's generation.
// A failure takes the rows' bits out of the mirror again: nothing has changed.
static int commit_fresh_deletes(vrod_index* idx, const std::vector<uint64_t>& fresh, uint64_t wlo, uint64_t whi) {
    if (fresh.empty()) return VROD_OK;
    int rc = set_device(idx);
    hipError_t e = hipSuccess;
    const bool first = !idx->del_dev.p;
    DevMem<uint32_t> first_dev;   // the first delete's device bitmap: the handle's once the upload is through
    if (rc == VROD_OK && first) {
        e = first_dev.alloc(idx->del_bits.size() * 4);
        wlo = 0; whi = idx->del_bits.size() - 1;   // the whole bitmap
    }
    uint32_t* const del_dev = first ? first_dev.p : idx->del_dev.p;
    if (rc == VROD_OK && e == hipSuccess)
        e = hipMemcpyAsync(del_dev + wlo, idx->del_bits.data() + wlo, (whi - wlo + 1) * 4, hipMemcpyHostToDevice, idx->stream);
    // under a filter: the rows this call deletes that were eligible leave the effective mask's zeros
    std::vector<uint32_t> eff_old;
    uint64_t lost = 0;
    if (idx->filter_on && rc == VROD_OK && e == hipSuccess) {
        eff_old.assign(idx->eff_bits.begin() + wlo, idx->eff_bits.begin() + whi + 1);
        for (uint64_t r : fresh) {
            uint32_t& w = idx->eff_bits[r / 32];
            const uint32_t bit = 1u << (r % 32);
            if (!(w & bit)) { w |= bit; ++lost; }
        }
        e = hipMemcpyAsync(idx->eff_dev.p + wlo, idx->eff_bits.data() + wlo, (whi - wlo + 1) * 4, hipMemcpyHostToDevice, idx->stream);
    }
    if (rc == VROD_OK && e == hipSuccess) e = hipStreamSynchronize(idx->stream);
    if (rc != VROD_OK || e != hipSuccess) {   // nothing changes: the mirrors forget this call's rows
        (void)hipStreamSynchronize(idx->stream);
        for (uint64_t r : fresh) idx->del_bits[r / 32] &= ~(1u << (r % 32));
        if (!eff_old.empty()) std::copy(eff_old.begin(), eff_old.end(), idx->eff_bits.begin() + wlo);
        if (!first) (void)hipMemcpy(del_dev + wlo, idx->del_bits.data() + wlo, (whi - wlo + 1) * 4, hipMemcpyHostToDevice);
        if (!eff_old.empty()) (void)hipMemcpy(idx->eff_dev.p + wlo, idx->eff_bits.data() + wlo, (whi - wlo + 1) * 4, hipMemcpyHostToDevice);
        return rc != VROD_OK ? rc : fail(e == hipErrorOutOfMemory ? VROD_ERR_OUT_OF_MEMORY : VROD_ERR_HIP, "uploading the deleted rows: %s", hipGetErrorString(e));
    }
    if (first) idx->del_dev.swap(first_dev);
    idx->n_deleted += fresh.size();
    if (idx->keys.exists())   // a deleted row's key is free: its slot goes stale, nothing is written to the table
        for (uint64_t r : fresh) idx->keyed_live -= idx->keys.host[r] != kKeyNone;
    idx->n_eligible -= lost;
    mask_changed(idx);
    return VROD_OK;
}

// Mark local rows (each < count) deleted: the host mirror, then the changed words on the device; under a filter the
// effective mask as well.
static int index_delete_rows(vrod_index* idx, const std::vector<uint64_t>& rows) {
    std::vector<uint64_t> fresh;   // rows this call deletes (repeats and rows deleted before are no-ops)
    uint64_t wlo = UINT64_MAX, whi = 0;
    for (uint64_t r : rows) {
        uint32_t& w = idx->del_bits[r / 32];
        const uint32_t bit = 1u << (r % 32);
        if (w & bit) continue;
        w |= bit;
        fresh.push_back(r);
        wlo = std::min(wlo, r / 32);
        whi = std::max(whi, r / 32);
    }
    return commit_fresh_deletes(idx, fresh, wlo, whi);
}

// ... and the rows of a hit bitmap (bit r set = local row r, live, dies; `words` words): what a delete by predicate
// gets from the device, one bit per row.
static int index_delete_hits(vrod_index* idx, const uint32_t* hits, uint64_t words, uint64_t* out_died) {
    std::vector<uint64_t> fresh;
    uint64_t wlo = UINT64_MAX, whi = 0;
    for (uint64_t w = 0; w < words; ++w) {
        const uint32_t h = hits[w] & ~idx->del_bits[w];   // (the pass's scope leaves deleted rows out already)
        if (!h) continue;
        idx->del_bits[w] |= h;
        for (uint32_t b = h; b; b &= b - 1u) fresh.push_back(w * 32 + (uint64_t)__builtin_ctz(b));
        wlo = std::min(wlo, w);
        whi = w;
    }
    VROD_TRY(commit_fresh_deletes(idx, fresh, wlo, whi));
    *out_died = fresh.size();
    return VROD_OK;
}

// Set (allow != null) or clear the filter of a single-device handle (or shard).  `allow`: n_rows bits (n_rows <= count),
// bit i set = local row i allowed.  Rows from n_rows on are not allowed.
static int index_set_filter(vrod_index* idx, const uint32_t* allow, uint64_t n_rows) {
    VROD_TRY(set_device(idx));
    if (!allow) {
        if (!idx->filter_on) return VROD_OK;
        idx->eff_dev.release();
        idx->filter_on = false;
        std::vector<uint32_t>().swap(idx->allow_bits);
        std::vector<uint32_t>().swap(idx->eff_bits);
        idx->n_eligible = 0;
        mask_changed(idx);
        return VROD_OK;
    }
    const size_t words = idx->del_bits.size();   // capacity / 32
    std::vector<uint32_t> al(words, 0u), eff(words, ~0u);
    const uint64_t full = n_rows / 32;
    for (uint64_t w = 0; w < full; ++w) al[w] = allow[w];
    if (n_rows % 32) al[full] = allow[full] & ((1u << (n_rows % 32)) - 1u);
    uint64_t n_el = 0;
    for (size_t w = 0; w < words; ++w) {
        eff[w] = idx->del_bits[w] | ~al[w];
        n_el += (uint64_t)__builtin_popcount(~eff[w]);   // (rows >= count are never allowed: n_rows <= count)
    }
    DevMem<uint32_t> first_dev;   // of the first filter since none was set: a later one is uploaded over the mask in place
    if (words && !idx->eff_dev.p) HIP_TRY(first_dev.alloc(words * 4));
    if (words) {
        const hipError_t e = hipMemcpy(first_dev.p ? first_dev.p : idx->eff_dev.p, eff.data(), words * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(VROD_ERR_HIP, "uploading the filter: %s", hipGetErrorString(e));
    }
    if (first_dev.p) idx->eff_dev.swap(first_dev);
    idx->allow_bits.swap(al);
    idx->eff_bits.swap(eff);
    idx->n_eligible = n_el;
    idx->filter_on = true;
    mask_changed(idx);
    return VROD_OK;
}

// A composite handle's filter: the bits name global ids; each shard gets the bits of its own local rows.  The global
// rows dealt to a shard are whole 65536-row blocks, so the bits move a 32-bit word at a time.
static int composite_set_filter(vrod_index* idx, const uint32_t* allow, uint64_t n_rows) {
    const size_t G = idx->shards.size();
    if (!allow) {
        for (vrod_index* sh : idx->shards) VROD_TRY(index_set_filter(sh, nullptr, 0));
        return VROD_OK;
    }
    std::vector<std::vector<uint32_t>> local(G);
    std::vector<uint64_t> local_n(G, 0);
    for (size_t g = 0; g < G; ++g) local[g].assign((idx->shards[g]->count + 31) / 32 + 1, 0u);
    (void)for_each_piece(idx, 0, n_rows, [&](size_t g, uint64_t r, uint64_t m) {
        const uint64_t lr = local_row_of(idx, r);   // r and lr are multiples of 32 (block starts), m is unless it is the last piece
        for (uint64_t i = 0; i < m; i += 32) {
            uint32_t w = allow[(r + i) / 32];
            if (m - i < 32) w &= (1u << (m - i)) - 1u;
            local[g][(lr + i) / 32] = w;
        }
        local_n[g] = lr + m;
        return (int)VROD_OK;
    });
    for (size_t g = 0; g < G; ++g) {
        const int rc = index_set_filter(idx->shards[g], local[g].data(), local_n[g]);
        if (rc != VROD_OK) {   // all or nothing: no shard keeps a filter
            const std::string why = g_last_error;
            for (vrod_index* sh : idx->shards) (void)index_set_filter(sh, nullptr, 0);
            g_last_error = why;
            return rc;
        }
    }
    return VROD_OK;
}

// ids -> (shard, local row) of a composite handle, every id checked before any shard changes
static int composite_delete(vrod_index* idx, const uint64_t* ids, uint64_t n) {
    std::vector<std::vector<uint64_t>> local(idx->shards.size());
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t r = ids[i] - idx->id_offset;
        local[(size_t)((r / kShardBlock) % idx->shards.size())].push_back(local_row_of(idx, r));
    }
    for (size_t g = 0; g < idx->shards.size(); ++g)
        if (!local[g].empty()) VROD_TRY(index_delete_rows(idx->shards[g], local[g]));
    return VROD_OK;
}

// An update of a composite handle: each row goes to the shard that holds its id.  Every shard checks its rows (NaN /
// Inf) before any shard writes one, so a rejected call changes nothing on the handle as a whole.
// rows_of: per row of the call its global row, skip[i]: the call names that id again later.  Each shard takes its rows
// of the source through a list of them.
static int composite_update(vrod_index* idx, const std::vector<uint64_t>& rows_of, const std::vector<bool>& skip, const RowSource& src) {
    const size_t G = idx->shards.size();
    std::vector<std::vector<uint32_t>> dst(G);
    std::vector<std::vector<uint64_t>> pick(G);
    for (size_t i = 0; i < rows_of.size(); ++i) {
        const uint64_t r = rows_of[i];
        const size_t g = (size_t)((r / kShardBlock) % G);
        dst[g].push_back(skip[i] ? kScatterSkip : (uint32_t)local_row_of(idx, r));
        pick[g].push_back(src.pick ? src.pick[i] : (uint64_t)i);
    }
    for (size_t g = 0; g < G; ++g)
        if (!dst[g].empty()) VROD_TRY(index_update_pass(idx->shards[g], nullptr, rows_picked(src, pick[g].data()), dst[g].size(), false));
    for (size_t g = 0; g < G; ++g)
        if (!dst[g].empty()) VROD_TRY(index_update_pass(idx->shards[g], dst[g].data(), rows_picked(src, pick[g].data()), dst[g].size(), false));
    return VROD_OK;
}

static int composite_get_rows(vrod_index* idx, uint64_t first, uint64_t n, float* out_rows) {
    return for_each_piece(idx, first, n, [&](size_t g, uint64_t r, uint64_t m) {
        return vrod_index_get_rows(idx->shards[g], local_row_of(idx, r), m, out_rows + (r - first) * idx->dim);
    });
}

// ---- RCCL, bound at run time.  A multi-device handle exchanges the per-shard top-k with ONE
// ncclAllGather per device inside a group call ("single process, ncclCommInitAll, one
// stream per device").  librccl is dlopen'ed when the first such handle is created: a process that
// already holds it (PyTorch ships one with the same soname) shares that copy, and single-device
// handles never load it.
struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;   // why it could not be loaded
};
static RcclApi& rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api;
    tried = true;
    // VROD_RCCL_LIB names THE library: when it is set nothing else is tried (a path that does not load means peer copies)
    const char* env = getenv("VROD_RCCL_LIB");
    const bool only_env = env && env[0];
    const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        if (!n || !n[0] || (only_env && n != env)) continue;
        api.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (api.h) break;
        api.why = dlerror();
    }
    if (!api.h) return api;
    bool ok = true;
    auto sym = [&](const char* name) { void* f = dlsym(api.h, name); if (!f) { ok = false; api.why = std::string("missing symbol ") + name; } return f; };
    api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    if (!ok) { dlclose(api.h); api.h = nullptr; }
    return api;
}
#define NCCL_TRY(expr)                                                                          \
    do {                                                                                        \
        ncclResult_t r_ = (expr);                                                               \
        if (r_ != ncclSuccess)                                                                  \
            return fail(VROD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, rccl_api().GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

// Groups the shards by device and opens the communicator over the distinct devices.
static int composite_open_exchange(vrod_index* idx) {
    for (size_t g = 0; g < idx->shards.size(); ++g) {
        const int dev = idx->shards[g]->device;
        size_t u = 0;
        while (u < idx->groups.size() && idx->groups[u].device != dev) ++u;
        if (u == idx->groups.size()) { idx->groups.emplace_back(); idx->groups.back().device = dev; }
        idx->shard_home.push_back({u, idx->groups[u].members.size()});
        idx->groups[u].members.push_back(g);
    }
    for (auto& G : idx->groups) {
        HIP_TRY(hipSetDevice(G.device));
        HIP_TRY(hipStreamCreateWithFlags(&G.xstream, hipStreamNonBlocking));
    }
    const char* e = getenv("VROD_RCCL");
    idx->use_rccl = !(e && e[0] == '0');   // VROD_RCCL=0: peer copies to the first device instead
    // peer access between the first device (where the lists are merged) and the others: best effort -- without it the
    // runtime stages cross-device copies through the host, slower but correct
    for (size_t u = 1; u < idx->groups.size(); ++u) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, idx->groups[0].device, idx->groups[u].device) == hipSuccess && can) {
            (void)hipSetDevice(idx->groups[0].device);
            (void)hipDeviceEnablePeerAccess(idx->groups[u].device, 0);   // (hipErrorPeerAccessAlreadyEnabled is fine)
            (void)hipSetDevice(idx->groups[u].device);
            (void)hipDeviceEnablePeerAccess(idx->groups[0].device, 0);
        }
        (void)hipGetLastError();
    }
    if (idx->use_rccl) {
        RcclApi& api = rccl_api();
        if (!api.h) {
            // no collective library: the exchange falls back to peer copies to the first device (stats.exchange = 2), said once
            static bool warned = false;
            if (!warned) fprintf(stderr, "vrod: librccl could not be loaded (%s); multi-device handles exchange their lists by peer copies "
                                         "(set VROD_RCCL_LIB to the library's path for the RCCL all-gather)\n", api.why.c_str());
            warned = true;
            idx->use_rccl = false;
            return VROD_OK;
        }
        std::vector<int> devs;
        for (auto& G : idx->groups) devs.push_back(G.device);
        std::vector<ncclComm_t> comms(devs.size(), nullptr);
        // RCCL prints a version banner on stdout at the first communicator of a process, and the host's
        // stdout is the command's result channel (SEARCHSIMILAR prints its hits there): stdout points at
        // /dev/null while the communicator is built (callers are single-threaded by contract)
        fflush(stdout);
        const int saved = dup(1), nul = open("/dev/null", O_WRONLY);
        if (saved >= 0 && nul >= 0) (void)dup2(nul, 1);
        const ncclResult_t ir = api.CommInitAll(comms.data(), (int)devs.size(), devs.data());
        fflush(stdout);
        if (saved >= 0) { (void)dup2(saved, 1); close(saved); }
        if (nul >= 0) close(nul);
        if (ir != ncclSuccess) {
            fprintf(stderr, "vrod: ncclCommInitAll over %zu devices failed (%s); this handle exchanges its lists by peer copies\n", devs.size(), api.GetErrorString(ir));
            idx->use_rccl = false;
            return VROD_OK;
        }
        for (size_t u = 0; u < devs.size(); ++u) idx->groups[u].comm = comms[u];
    }
    return VROD_OK;
}

static size_t composite_lists_per_device(const vrod_index* idx) {
    size_t m = 1;
    for (auto& G : idx->groups) m = std::max(m, G.members.size());
    return m;
}
// one device's packed result block: nk ids (u64) then nk scores (f32), padded so that every list of
// the gathered buffer starts 16-B aligned whatever the parity of nq*k
static size_t composite_block_bytes(size_t nk) { return round_up(nk * 12, 16); }

// The shards' searches of the slot being begun: queries from the host (from_host), from device
// memory of the first device (d/h pointer `queries`), or rows of the synthetic stream (`queries`
// null).  Returns with every shard's search enqueued, or with none pending on an error.
static int composite_begin(vrod_index* idx, const float* queries, bool from_host, uint64_t seed, uint64_t first_row,
                           uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores, void* caller_stream) {
    if (idx->n_pending() >= 2) return fail(VROD_ERR_INVALID_ARG, "two searches are already pending: call vrod_search_end first");
    const uint32_t c = idx->n_begun & 1;
    vrod_index::CompPending& CP = idx->cslot[c];
    CP.nq = nq; CP.k = k; CP.out_ids = out_ids; CP.out_scores = out_scores;
    const size_t G = idx->shards.size(), U = idx->groups.size();
    const size_t nk = (size_t)nq * k, block = composite_block_bytes(nk), M = composite_lists_per_device(idx);
    const size_t qbytes = (size_t)nq * idx->dim * 4;
    idx->sh_q[c].resize(G);
    if (nq) {
        for (size_t u = 0; u < U; ++u) {
            vrod_index::DevGroup& D = idx->groups[u];
            VROD_TRY(set_device(idx->shards[D.members[0]]));
            const void* before = D.send[c].p;
            VROD_TRY(D.send[c].ensure(M * block));
            VROD_TRY(D.recv[c].ensure(U * M * block));
            if (D.members.size() < M && (D.send[c].p != before || D.filled_nk[c] != nk + 1)) {
                // list slots no shard of this device writes: "no result" entries, which the merge skips
                for (size_t m = D.members.size(); m < M; ++m)
                    launch_fill_none((uint64_t*)((char*)D.send[c].p + m * block), (float*)((char*)D.send[c].p + m * block + nk * 8), nk, D.xstream);
                HIP_TRY(hipStreamSynchronize(D.xstream));
                D.filled_nk[c] = nk + 1;
            }
        }
        if (queries && !from_host) {   // the caller's stream (first device) produced the queries
            VROD_TRY(set_device(idx->shards[idx->groups[0].members[0]]));
            if (!idx->caller_ev) HIP_TRY(hipEventCreateWithFlags(&idx->caller_ev, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(idx->caller_ev, (hipStream_t)caller_stream));
        }
    }
    // Device outputs (both device forms, the synthetic one included): whatever the caller's stream still does with the
    // buffers of an earlier batch -- a kernel reading its results -- comes before the merge that overwrites them.
    // (The single-device path has the same ordering through order_after_caller.)
    CP.ordered = false;
    if (nq && !from_host && out_ids) {
        VROD_TRY(set_device(idx->shards[idx->groups[0].members[0]]));
        if (!CP.caller_ev) HIP_TRY(hipEventCreateWithFlags(&CP.caller_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(CP.caller_ev, (hipStream_t)caller_stream));
        CP.ordered = true;
    }
    int rc = VROD_OK;
    size_t begun = 0;
    for (size_t g = 0; g < G && rc == VROD_OK; ++g) {
        vrod_index* sh = idx->shards[g];
        const auto [u, m] = idx->shard_home[g];
        if ((rc = set_device(sh)) != VROD_OK) break;
        sh->path = idx->path;
        sh->profiling = idx->profiling;
        sh->deal = IdMap{idx->id_offset, (uint32_t)kShardBlock, (uint32_t)g, (uint32_t)G};
        uint64_t* oi = nq ? (uint64_t*)((char*)idx->groups[u].send[c].p + m * block) : nullptr;
        float* os = nq ? (float*)((char*)idx->groups[u].send[c].p + m * block + nk * 8) : nullptr;
        hipStream_t ss = next_slot(sh).stream;
        const float* q = nullptr;
        if (nq) {
            if ((rc = idx->sh_q[c][g].ensure(std::max<size_t>(qbytes, 4))) != VROD_OK) break;
            q = idx->sh_q[c][g].as<float>();
            hipError_t e = hipSuccess;
            if (!queries) {
                launch_synth_rows(seed, first_row, nq, idx->dim, idx->sh_q[c][g].as<float>(), ss);
            } else if (from_host) {
                e = hipMemcpyAsync(idx->sh_q[c][g].p, queries, qbytes, hipMemcpyHostToDevice, ss);
            } else {
                e = hipStreamWaitEvent(ss, idx->caller_ev, 0);
                if (e == hipSuccess) e = hipMemcpyAsync(idx->sh_q[c][g].p, queries, qbytes, hipMemcpyDefault, ss);
            }
            if (e != hipSuccess) { rc = fail(VROD_ERR_HIP, "queries to device %d: %s", sh->device, hipGetErrorString(e)); break; }
        }
        rc = search_begin(sh, q, nq, k, oi, os);
        if (rc == VROD_OK) ++begun;
    }
    if (rc != VROD_OK) {   // a search begun must be ended: nothing stays pending behind an error
        const std::string why = g_last_error;
        for (size_t g = 0; g < begun; ++g) { (void)set_device(idx->shards[g]); (void)search_end(idx->shards[g]); }
        g_last_error = why;
        return rc;
    }
    idx->n_begun++;
    return VROD_OK;
}

// Complete the oldest composite search: every shard's search, then the exchange (RCCL all-gather of
// one packed block per device, or peer copies with VROD_RCCL=0) and the merge on the first device.
// to_host: the caller's outputs are host memory (vrod_search).
static int composite_end(vrod_index* idx, uint64_t* host_ids, float* host_scores) {
    if (idx->n_pending() == 0) return fail(VROD_ERR_INVALID_ARG, "no search is pending");
    const uint32_t c = idx->n_ended & 1;
    idx->n_ended++;
    vrod_index::CompPending& CP = idx->cslot[c];
    const uint32_t nq = CP.nq, k = CP.k;
    const size_t G = idx->shards.size(), U = idx->groups.size();
    idx->stats = vrod_search_stats{};
    idx->stats.nq = nq;
    idx->stats.k = k;
    int rc = VROD_OK;
    for (size_t g = 0; g < G; ++g) {
        vrod_index* sh = idx->shards[g];
        const int r0 = set_device(sh);
        const int r = r0 != VROD_OK ? r0 : search_end(sh);     // every begun search is ended, whatever the others return
        if (r != VROD_OK && rc == VROD_OK) rc = r;
        const vrod_search_stats& st = sh->stats;
        idx->stats.path = st.path; idx->stats.kprime = st.kprime;
        idx->stats.scan_launches += st.scan_launches;
        idx->stats.fallback_queries += st.fallback_queries;
        idx->stats.band_queries += st.band_queries;
        idx->stats.split_pass |= st.split_pass;
        if (st.scan_ms > idx->stats.scan_ms) { idx->stats.sample_ms = st.sample_ms; idx->stats.overlap_ms = st.overlap_ms; }   // of the shard whose scans took longest
        idx->stats.scan_ms = std::max(idx->stats.scan_ms, st.scan_ms);
        idx->stats.total_ms = std::max(idx->stats.total_ms, st.total_ms);
        idx->stats.scan_bytes += st.scan_bytes; idx->stats.scan_flops += st.scan_flops;
        idx->stats.max_fast_err = std::max(idx->stats.max_fast_err, st.max_fast_err);
        idx->stats.eps_bound = std::max(idx->stats.eps_bound, st.eps_bound);
    }
    idx->stats.exchange = idx->use_rccl ? 1u : 2u;
    if (rc != VROD_OK || !nq) return rc;
    // every shard's list is complete in its device's send block (the host has seen each search end)
    const size_t nk = (size_t)nq * k, block = composite_block_bytes(nk), M = composite_lists_per_device(idx);
    vrod_index::DevGroup& D0 = idx->groups[0];
    if (idx->use_rccl) {
        RcclApi& api = rccl_api();
        NCCL_TRY(api.GroupStart());
        for (size_t u = 0; u < U; ++u) {
            vrod_index::DevGroup& D = idx->groups[u];
            const ncclResult_t r = api.AllGather(D.send[c].p, D.recv[c].p, M * block, ncclUint8, D.comm, D.xstream);
            if (r != ncclSuccess) { (void)api.GroupEnd(); return fail(VROD_ERR_HIP, "ncclAllGather failed: %s", api.GetErrorString(r)); }
        }
        NCCL_TRY(api.GroupEnd());
    } else {
        HIP_TRY(hipSetDevice(D0.device));
        for (size_t u = 0; u < U; ++u)
            HIP_TRY(hipMemcpyPeerAsync((char*)D0.recv[c].p + u * M * block, D0.device, idx->groups[u].send[c].p, idx->groups[u].device, M * block, D0.xstream));
    }
    HIP_TRY(hipSetDevice(D0.device));
    if (CP.ordered) HIP_TRY(hipStreamWaitEvent(D0.xstream, CP.caller_ev, 0));   // the caller's earlier use of the output buffers
    uint64_t* oi = CP.out_ids;
    float* os = CP.out_scores;
    if (host_ids) {
        VROD_TRY(idx->out_ids.ensure(nk * 8));
        VROD_TRY(idx->out_scores.ensure(nk * 4));
        oi = idx->out_ids.as<uint64_t>();
        os = idx->out_scores.as<float>();
    }
    launch_merge_topk(score_form(idx->metric), (const uint64_t*)D0.recv[c].p, (const float*)((const char*)D0.recv[c].p + nk * 8), block / 8, block / 4,
                      (uint32_t)(U * M), nq, k, oi, os, D0.xstream);
    HIP_TRY(hipGetLastError());
    if (host_ids) {
        HIP_TRY(hipMemcpyAsync(host_ids, oi, nk * 8, hipMemcpyDeviceToHost, D0.xstream));
        HIP_TRY(hipMemcpyAsync(host_scores, os, nk * 4, hipMemcpyDeviceToHost, D0.xstream));
    }
    // the other devices' all-gathers read their send blocks: done before the slot is reused
    for (size_t u = U; u-- > 0;) {
        HIP_TRY(hipSetDevice(idx->groups[u].device));
        HIP_TRY(hipStreamSynchronize(idx->groups[u].xstream));
    }
    return VROD_OK;
}

static int composite_search(vrod_index* idx, const float* queries, bool from_host, uint64_t seed, uint64_t first_row, uint32_t nq, uint32_t k,
                            uint64_t* out_ids, float* out_scores, void* caller_stream) {
    if (idx->n_pending()) return fail(VROD_ERR_INVALID_ARG, "a synchronous search while a search is pending: call vrod_search_end first");
    VROD_TRY(composite_begin(idx, queries, from_host, seed, first_row, nq, k, from_host ? nullptr : out_ids, from_host ? nullptr : out_scores, caller_stream));
    return composite_end(idx, from_host ? out_ids : nullptr, from_host ? out_scores : nullptr);
}

// ------------------------------------------------------------------ range search
// Every eligible row whose canonical score is at least as good as the caller's per-query threshold (DESIGN.md scan
// spec rule 10).  A range search is synchronous: it runs in the slot the next search would take, on a handle with
// nothing pending, and leaves the slot as it found it (no candidate margin, split-pass or graph state is touched).
//
//   fast route       thresholds widened by the error bound (range_prepare_kernel), ONE filtered MFMA launch over the
//                    whole corpus into the slot's list block, counters read back; a list that overflowed means the
//                    row range is redone in pieces (search_plan.h range_split); every completed range is re-scored
//                    canonically and cut at the caller's threshold (range_rescore_cut_kernel)
//   canonical route  the queries without a finite bound, VROD_PATH_EXACT, and the gather route of a narrow filter:
//                    canonical scores of all (eligible) rows through the exact path's kernels, cut the same way
// Both append to the shard's pool and count per query; ordering and output are the caller's (range_emit).
struct RangeShardResult {
    std::vector<uint64_t> counts;   // qualifying rows per query
    uint64_t total = 0, stored = 0; // their sum; entries in the shard's pool (unsorted), min(total, pool capacity)
};

static int range_collect(vrod_index* idx, const float* d_queries_raw, uint32_t nq, const float* h_thresholds, uint64_t capacity,
                         RangeShardResult& R) {
    VROD_TRY(set_device(idx));
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    vrod_search_stats& st = P.st;
    st = vrod_search_stats{};
    st.nq = nq;
    R.counts.assign(nq, 0);
    R.total = R.stored = 0;
    P.ev_used = 0; P.t0 = P.t1 = 0; P.scan_pairs.clear(); P.sample_pair = -1; P.tail_pair = -1;
    P.gkey_valid = false;   // the slot's workspaces may move: a search seen before is seen afresh
    const uint64_t N = idx->count;
    const int form = score_form(idx->metric);
    // the route: STREAM has no threshold form (treated as AUTO); the filter route decides as it does for a search
    const int forced = idx->path == VROD_PATH_STREAM ? VROD_PATH_AUTO : idx->path;
    const bool gather = forced == VROD_PATH_GATHER || (idx->filter_on && filter_route(forced, idx->dtype, N, idx->eligible(), nq, idx->dim));
    const bool exact = !gather && forced == VROD_PATH_EXACT;
    const bool fast = !gather && !exact;
    st.path = gather ? VROD_PATH_GATHER : exact ? VROD_PATH_EXACT : VROD_PATH_MFMA;
    if (N == 0 || idx->eligible() == 0) { idx->stats = st; return VROD_OK; }
    const bool split = fast && idx->dtype == VROD_DTYPE_F32 && idx->split_enabled && planes_ready(idx);
    P.plan = make_range_plan(split, form, idx->dim, N, nq);
    P.plan.path = (int)st.path;
    const SearchPlan& plan = P.plan;
    st.split_pass = split ? 1u : 0u;
    Timer tm(idx, P);
    P.t0 = tm.mark();

    // ---- workspaces; the caller's thresholds and zeroed counters on the device
    const uint32_t nq_pad = plan.nq_pad, cap = kSelectChunk;
    VROD_TRY(P.q_f32.ensure((size_t)nq_pad * idx->ld * 4));
    void* q_lp = nullptr;
    if (idx->dtype == VROD_DTYPE_BF16) {
        VROD_TRY(P.q_lp.ensure((size_t)nq_pad * idx->ld * 2));
        q_lp = P.q_lp.p;
    }
    VROD_TRY(P.small.ensure(small_bytes(nq_pad)));
    if (fast) VROD_TRY(P.lists.ensure(list_bytes(nq_pad)));
    VROD_TRY(idx->range_small.ensure(8 + (size_t)nq * 8));
    const uint64_t pool_cap = std::min<uint64_t>(capacity, (uint64_t)nq * idx->eligible());
    if (pool_cap) VROD_TRY(idx->range_pool.ensure((size_t)pool_cap * sizeof(RangeHit)));
    RangePool pool{idx->range_pool.as<RangeHit>(), pool_cap, idx->range_small.as<unsigned long long>(), nullptr};
    float* d_thr = (float*)((char*)idx->range_small.p + 8);
    pool.per_query = (uint32_t*)(d_thr + nq);
    HIP_TRY(hipMemsetAsync(idx->range_small.p, 0, 8 + (size_t)nq * 8, s));
    HIP_TRY(hipMemcpyAsync(d_thr, h_thresholds, (size_t)nq * 4, hipMemcpyHostToDevice, s));

    // ---- prepare the queries exactly as a search does (the same launch resets the list counters and pacing regions)
    const SmallBlock B = small_block(P);
    QueryInit qi{};
    qi.status = B.status;
    qi.counts = fast ? list_block(P).counts : nullptr;
    qi.thr = fast ? B.thr : nullptr;
    qi.thr_live_bits = qi.thr_pad_bits = form == M_COSINE ? 0x7F800000u : 0xFF800000u;   // nothing passes until range_prepare
    qi.zero_words2 = fast ? pace_region(P, 0) : nullptr;
    qi.n_zero_words2 = kPaceRegions * (kPaceWords + kClaimWords);
    // (prep_ovr: a near-duplicate batch's queries are stored rows, taken as given -- negative for every other caller)
    launch_prep_queries(d_queries_raw, nq, nq_pad, idx->dim, idx->ld, idx->prep_ovr >= 0 ? idx->prep_ovr : prep_form(idx->metric), idx->dtype,
                        P.q_f32.as<float>(), q_lp, B.qn2, &P.flags.p[0], &P.flags.p[1], qi, s);
    if (fast)
        launch_range_prepare(d_thr, nq, nq_pad, form, plan.eps_mode, plan.eps_c, &P.flags.p[1], idx->max_xn2_bits, B.thr, B.status, s);
    HIP_TRY(hipGetLastError());

    // whatever happens from here on, the slot's per-search scalars (bad-value flag, max |q|^2, max error) end up consumed
    struct FlagReset {
        Pending& P;
        ~FlagReset() { (void)hipMemsetAsync(&P.flags.p[0], 0, 12, P.stream); (void)hipStreamSynchronize(P.stream); }
    } flag_reset{P};

    std::vector<uint32_t> canon_q;   // queries of the canonical (dense) route
    std::vector<uint32_t> hcnt(nq), hcanon(nq, 0u);
    uint32_t hflags[2] = {0u, 0u};
    auto check_queries = [&]() -> int {
        if (hflags[0]) { idx->stats = st; return fail(VROD_ERR_INVALID_VALUE, "queries contain NaN or Inf"); }
        return VROD_OK;
    };
    if (fast) {
        MfmaScanArgs a;
        VROD_TRY(mfma_args(idx, P, a, idx->dtype == VROD_DTYPE_BF16 ? q_lp : P.q_f32.p, B.qn2, B.thr, nq, nq_pad));
        if (split) {
            if (idx->planes_rows < N) {   // planes of the rows added since the last batched search (as mfma_pass)
                launch_split_rows((const float*)idx->corpus.p + idx->planes_rows * idx->ld, N - idx->planes_rows, idx->ld, idx->ldp,
                                  (char*)idx->planes.p + idx->planes_rows * 2ull * idx->ldp * 2ull, false, s);
                if (round_up(N, kRowTile) > N)
                    HIP_TRY(hipMemsetAsync((char*)idx->planes.p + N * 2ull * idx->ldp * 2ull, 0, (round_up(N, kRowTile) - N) * 2ull * idx->ldp * 2ull, s));
                idx->planes_rows = N;
            }
            VROD_TRY(use_split_planes(idx, a, P.q_f32.as<float>(), nq_pad, P.q_planes, s));
        }
        const int scan_dtype = split ? VROD_DTYPE_BF16 : idx->dtype;
        const ListBlock L = list_block(P);
        P.pace_launches = 0;
        // row ranges still to scan, in row order: the whole corpus first; a range whose fullest list overflowed is
        // replaced by its pieces.  A one-tile range appends at most 256 rows per query: the loop terminates.
        std::vector<std::pair<uint64_t, uint64_t>> todo{{0, N}};
        bool first = true;
        while (!todo.empty()) {
            const std::pair<uint64_t, uint64_t> rg = todo.back();
            todo.pop_back();
            if (!first) HIP_TRY(hipMemsetAsync(L.counts, 0, (size_t)nq_pad * 4, s));
            launch_filtered(idx, P, tm, a, scan_dtype, rg.first, rg.second, true, false);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(hcnt.data(), L.counts, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
            if (first) {
                HIP_TRY(hipMemcpyAsync(hcanon.data(), B.status, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(hflags, &P.flags.p[0], 8, hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(hipStreamSynchronize(s));
            if (first) VROD_TRY(check_queries());
            first = false;
            uint32_t maxc = 0;
            for (uint32_t c : hcnt) maxc = std::max(maxc, c);
            if (maxc > cap) {
                const std::vector<uint64_t> b = range_split(rg.first, rg.second, maxc, cap);
                if (b.size() < 3) { idx->stats = st; return fail(VROD_ERR_INTERNAL, "a hit list of one tile overflowed (%u entries)", maxc); }
                for (size_t i = b.size() - 1; i > 0; --i) todo.push_back({b[i - 1], b[i]});
                continue;
            }
            st.kprime = std::max(st.kprime, maxc);
            launch_range_rescore_cut(idx->corpus.p, idx->dtype, form, idx->dim, idx->ld, P.q_f32.as<float>(), nq, L.lists, L.counts, cap, maxc, d_thr,
                                     idmap_of(idx), pool, &P.flags.p[2], s);
            HIP_TRY(hipGetLastError());
        }
        for (uint32_t q = 0; q < nq; ++q)
            if (hcanon[q]) canon_q.push_back(q);
        st.fallback_queries = (uint32_t)canon_q.size();
    } else {
        HIP_TRY(hipMemcpyAsync(hflags, &P.flags.p[0], 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        VROD_TRY(check_queries());
        if (exact) {
            for (uint32_t q = 0; q < nq; ++q) canon_q.push_back(q);
            st.fallback_queries = nq;
        }
    }

    // ---- canonical route, dense form: up to 8 queries share one pass over the corpus (the exact path's kernel)
    if (!canon_q.empty()) {
        const uint64_t score_ld = round_up(N, 64);
        int gmax = rescore_all_max_queries(idx->ld);
        while (gmax > 1 && (uint64_t)gmax * score_ld * 4 > (1ull << 30)) gmax >>= 1;
        for (size_t f0 = 0; f0 < canon_q.size();) {
            int g = gmax;
            while ((size_t)g > canon_q.size() - f0) g >>= 1;
            VROD_TRY(P.scores.ensure((size_t)g * score_ld * 4));
            launch_rescore_all(idx->corpus.p, idx->dtype, form, idx->dim, idx->ld, P.q_f32.as<float>(), &canon_q[f0], g, N, P.scores.as<float>(), score_ld, s);
            launch_range_cut_scores(P.scores.as<float>(), score_ld, N, (uint32_t)g, &canon_q[f0], 0, form, d_thr, idx->row_mask(), nullptr, idmap_of(idx), pool, s);
            HIP_TRY(hipGetLastError());
            if (!fast) { st.scan_launches++; st.scan_bytes += (double)N * idx->ld * idx->esize; st.scan_flops += 2.0 * g * (double)N * idx->dim; }
            f0 += g;
        }
    }
    // ---- canonical route, list form: the eligible rows only (the gather path's kernel)
    if (gather) {
        VROD_TRY(gather_list(idx));
        const uint64_t m = idx->list_n;
        const uint64_t score_ld = round_up(m, 64);
        uint64_t g = std::max<uint64_t>(1, (1ull << 30) / (score_ld * 4));
        if (g >= nq) g = nq;
        else if (g > 8) g = g / 8 * 8;
        VROD_TRY(P.scores.ensure((size_t)g * score_ld * 4));
        for (uint32_t q0 = 0; q0 < nq; q0 += (uint32_t)g) {
            const uint32_t gc = (uint32_t)std::min<uint64_t>(g, nq - q0);
            launch_rescore_list(idx->corpus.p, idx->dtype, form, idx->dim, idx->ld, P.q_f32.as<float>() + (size_t)q0 * idx->ld, gc, idx->list_dev.as<uint32_t>(), m,
                                P.scores.as<float>(), score_ld, s);
            launch_range_cut_scores(P.scores.as<float>(), score_ld, m, gc, nullptr, q0, form, d_thr, nullptr, idx->list_dev.as<uint32_t>(), idmap_of(idx), pool, s);
            HIP_TRY(hipGetLastError());
            st.scan_launches++;
        }
        st.scan_bytes = (double)m * idx->ld * idx->esize;
        st.scan_flops = 2.0 * nq * (double)m * idx->dim;
    }

    // ---- counters back
    std::vector<uint32_t> hq(nq);
    unsigned long long htotal = 0;
    uint32_t herr = 0, hmaxx = 0;
    HIP_TRY(hipMemcpyAsync(hq.data(), pool.per_query, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&htotal, pool.n_total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&herr, &P.flags.p[2], 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&hmaxx, idx->max_xn2_bits, 4, hipMemcpyDeviceToHost, s));
    P.t1 = tm.mark();
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t q = 0; q < nq; ++q) R.counts[q] = hq[q];
    R.total = htotal;
    R.stored = std::min<uint64_t>(htotal, pool_cap);
    if (fast && canon_q.size() < nq) {   // a fast pass ran for some query
        memcpy(&st.max_fast_err, &herr, 4);
        float qn2, xn2;
        memcpy(&qn2, &hflags[1], 4);
        memcpy(&xn2, &hmaxx, 4);
        st.eps_bound = eps_bound(plan.eps_mode, plan.eps_c, qn2, xn2);
    }
    if (idx->profiling) {
        for (size_t i = 0; i < P.scan_pairs.size(); ++i) st.scan_ms += tm.pair_ms(i);
        if (idx->profiling >= 2) st.total_ms = tm.ms(P.t0, P.t1);
    }
    idx->stats = st;
    return VROD_OK;
}

// Order `n` pool entries (device memory of the current device, d_pool; d_tmp its sort partner) and write them to the
// caller's arrays: device pointers, or host pointers through the handle's staging buffers.
static int range_emit(vrod_index* idx, RangeHit* d_pool, RangeHit* d_tmp, uint64_t n, uint64_t* out_ids, float* out_scores, bool to_host, hipStream_t s) {
    if (!n) return VROD_OK;
    const RangeHit* sorted = launch_range_sort(d_pool, d_tmp, n, s);
    uint64_t* oi = out_ids;
    float* os = out_scores;
    if (to_host) {
        VROD_TRY(idx->out_ids.ensure((size_t)n * 8));
        VROD_TRY(idx->out_scores.ensure((size_t)n * 4));
        oi = idx->out_ids.as<uint64_t>();
        os = idx->out_scores.as<float>();
    }
    launch_range_emit(sorted, n, score_form(idx->metric), oi, os, s);
    HIP_TRY(hipGetLastError());
    if (to_host) {
        HIP_TRY(hipMemcpyAsync(out_ids, oi, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out_scores, os, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return VROD_OK;
}

// The whole call.  `queries` / outputs: host pointers (to_host) or device pointers on the handle's first device; the
// thresholds are on the host by now (validated).  h_lims [nq + 1] is always filled once the scan ran.
static int range_search(vrod_index* idx, const float* queries, bool from_host, uint32_t nq, const float* h_thresholds, uint64_t capacity,
                        uint64_t* h_lims, uint64_t* out_ids, float* out_scores) {
    const size_t qbytes = (size_t)nq * idx->dim * 4;
    std::vector<uint64_t> counts(nq, 0);
    uint64_t total = 0;
    std::vector<RangeShardResult> res(idx->composite() ? idx->shards.size() : 1);
    if (!idx->composite()) {
        VROD_TRY(set_device(idx));
        Pending& P = next_slot(idx);
        const float* dq = queries;
        if (from_host) {
            VROD_TRY(P.q_raw.ensure(qbytes));
            HIP_TRY(hipMemcpyAsync(P.q_raw.p, queries, qbytes, hipMemcpyHostToDevice, P.stream));
            dq = P.q_raw.as<float>();
        }
        VROD_TRY(range_collect(idx, dq, nq, h_thresholds, capacity, res[0]));
        counts = res[0].counts;
        total = res[0].total;
    } else {
        // every shard answers the same thresholds over its own rows (one after the other); counts add up
        const size_t G = idx->shards.size();
        vrod_search_stats agg{};
        agg.nq = nq;
        for (size_t g = 0; g < G; ++g) {
            vrod_index* sh = idx->shards[g];
            VROD_TRY(set_device(sh));
            sh->path = idx->path;
            sh->profiling = idx->profiling;
            sh->deal = IdMap{idx->id_offset, (uint32_t)kShardBlock, (uint32_t)g, (uint32_t)G};
            Pending& P = next_slot(sh);
            VROD_TRY(P.q_raw.ensure(qbytes));
            HIP_TRY(hipMemcpyAsync(P.q_raw.p, queries, qbytes, from_host ? hipMemcpyHostToDevice : hipMemcpyDefault, P.stream));
            VROD_TRY(range_collect(sh, P.q_raw.as<float>(), nq, h_thresholds, capacity, res[g]));
            for (uint32_t q = 0; q < nq; ++q) counts[q] += res[g].counts[q];
            total += res[g].total;
            const vrod_search_stats& st = sh->stats;
            agg.path = st.path;
            agg.kprime = std::max(agg.kprime, st.kprime);
            agg.scan_launches += st.scan_launches;
            agg.fallback_queries = std::max(agg.fallback_queries, st.fallback_queries);   // (the same queries on every shard)
            agg.split_pass |= st.split_pass;
            agg.scan_ms = std::max(agg.scan_ms, st.scan_ms);
            agg.total_ms += st.total_ms;
            agg.scan_bytes += st.scan_bytes; agg.scan_flops += st.scan_flops;
            agg.max_fast_err = std::max(agg.max_fast_err, st.max_fast_err);
            agg.eps_bound = std::max(agg.eps_bound, st.eps_bound);
        }
        agg.exchange = 2u;   // peer copies
        idx->stats = agg;
    }
    h_lims[0] = 0;
    for (uint32_t q = 0; q < nq; ++q) h_lims[q + 1] = h_lims[q] + counts[q];
    if (total > capacity)
        return fail(VROD_ERR_CAPACITY, "%llu rows qualify, the buffers hold %llu", (unsigned long long)total, (unsigned long long)capacity);
    if (!total) return VROD_OK;
    if (!idx->composite()) {
        VROD_TRY(idx->range_pool_b.ensure((size_t)total * sizeof(RangeHit)));
        return range_emit(idx, idx->range_pool.as<RangeHit>(), idx->range_pool_b.as<RangeHit>(), total, out_ids, out_scores, from_host, next_slot(idx).stream);
    }
    // the shards' pools gathered on the first device (peer copies) and ordered there as one: (query, score, GLOBAL id)
    vrod_index::DevGroup& D0 = idx->groups[0];
    HIP_TRY(hipSetDevice(D0.device));
    VROD_TRY(idx->range_pool.ensure((size_t)total * sizeof(RangeHit)));
    VROD_TRY(idx->range_pool_b.ensure((size_t)total * sizeof(RangeHit)));
    uint64_t at = 0;
    for (size_t g = 0; g < idx->shards.size(); ++g) {
        if (!res[g].stored) continue;
        HIP_TRY(hipMemcpyPeerAsync(idx->range_pool.as<RangeHit>() + at, D0.device, idx->shards[g]->range_pool.p, idx->shards[g]->device,
                                   (size_t)res[g].stored * sizeof(RangeHit), D0.xstream));
        at += res[g].stored;
    }
    return range_emit(idx, idx->range_pool.as<RangeHit>(), idx->range_pool_b.as<RangeHit>(), total, out_ids, out_scores, from_host, D0.xstream);
}

static int check_range_args(vrod_index* idx, const void* q, uint32_t nq, const void* thr, uint64_t capacity, const void* lims, const void* oi, const void* os) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    if (!lims) return fail(VROD_ERR_INVALID_ARG, "out_lims is null");
    if (nq && (!q || !thr)) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    if (capacity && (!oi || !os)) return fail(VROD_ERR_INVALID_ARG, "capacity %llu with a null output buffer", (unsigned long long)capacity);
    if (idx->n_pending()) return fail(VROD_ERR_INVALID_ARG, "vrod_range_search while a search is pending: call vrod_search_end first");
    return VROD_OK;
}
static int check_thresholds(const float* h_thr, uint32_t nq) {
    for (uint32_t q = 0; q < nq; ++q)
        if (h_thr[q] != h_thr[q]) return fail(VROD_ERR_INVALID_VALUE, "threshold %u is NaN", q);
    return VROD_OK;
}

// ------------------------------------------------------------------ the steps of the searches over groups of rows
// A dense group's stats folded into the call's.
static void fold_stats(vrod_search_stats& st, const vrod_search_stats& d) {
    st.path = d.path;
    st.kprime = std::max(st.kprime, d.kprime);
    st.scan_launches += d.scan_launches;
    st.fallback_queries += d.fallback_queries;
    st.band_queries += d.band_queries;
    st.max_fast_err = std::max(st.max_fast_err, d.max_fast_err);
    st.eps_bound = std::max(st.eps_bound, d.eps_bound);
    st.scan_ms += d.scan_ms;
    st.sample_ms += d.sample_ms;
    st.total_ms += d.total_ms;
    st.split_pass |= d.split_pass;
}

// The steps the synchronous searches over groups of queries share (labelled, tagged, grouped, multi-vector).
// No eligible row can answer: every result slot unfilled (as vrod_search), the stream drained, `st` the call's stats.
static int return_unfilled(vrod_index* idx, hipStream_t s, const vrod_search_stats& st, uint64_t* d_out_ids, float* d_out_scores, uint64_t n) {
    launch_fill_none(d_out_ids, d_out_scores, n, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    idx->stats = st;
    return VROD_OK;
}

// Prepare the batch's queries into P.q_f32 as a search does; NaN / Inf fails the call before anything is scored.
static int prep_queries_checked(vrod_index* idx, Pending& P, const float* d_queries_raw, uint32_t nq) {
    hipStream_t s = P.stream;
    P.plan = SearchPlan{};
    P.plan.nq_pad = nq;
    VROD_TRY(P.q_f32.ensure((size_t)nq * idx->ld * 4));
    VROD_TRY(P.small.ensure(small_bytes(nq)));
    const SmallBlock B = small_block(P);
    QueryInit qi{};
    qi.status = B.status;
    launch_prep_queries(d_queries_raw, nq, nq, idx->dim, idx->ld, prep_form(idx->metric), idx->dtype, P.q_f32.as<float>(), nullptr, B.qn2,
                        &P.flags.p[0], &P.flags.p[1], qi, s);
    launch_gather_readback(B.status, nq, P.flags.p, idx->max_xn2_bits, B.readback, s);   // (consumes the slot's scalars)
    HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, B.readback + nq, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return fail(VROD_ERR_INVALID_VALUE, "queries contain NaN or Inf");
    return VROD_OK;
}

// The two passes over the label array (kernels_label.hip) for up to Gc labels at a time.  Their workspace: lab_tab as
// [table | totals | segment offsets], Gc words each, and the per-block counts in lab_cnt.
struct LabelPassWs { uint32_t rpb; uint32_t* table; uint32_t* total; uint32_t* seg_off; uint32_t* cnt; };
static int label_pass_ws(vrod_index* idx, uint32_t Gc, LabelPassWs& W) {
    const uint32_t rpb = label_rows_per_block(idx->count);
    const uint32_t n_blocks = (uint32_t)((idx->count + rpb - 1) / rpb);
    VROD_TRY(idx->lab_tab.ensure((size_t)Gc * 4 * 3));
    VROD_TRY(idx->lab_cnt.ensure((size_t)n_blocks * Gc * 4));
    uint32_t* t = idx->lab_tab.as<uint32_t>();
    W = LabelPassWs{rpb, t, t + Gc, t + 2 * (size_t)Gc, idx->lab_cnt.as<uint32_t>()};
    return VROD_OK;
}
// Pass 1: the eligible rows of each of the Gp labels h_table, counted per block of the label array and in all.
// h_total: the totals are read back into it, and the stream is drained; null: the launch is only enqueued.
static int label_count_pass(vrod_index* idx, hipStream_t s, const LabelPassWs& W, const uint32_t* h_table, uint32_t Gp, uint32_t* h_total) {
    HIP_TRY(hipMemcpyAsync(W.table, h_table, (size_t)Gp * 4, hipMemcpyHostToDevice, s));
    launch_label_group_count(idx->labels.d(), idx->row_mask(), idx->count, W.rpb, W.table, Gp, W.cnt, Gp, s);
    launch_group_prefix(W.cnt, (uint32_t)((idx->count + W.rpb - 1) / W.rpb), Gp, W.total, s);
    if (!h_total) return VROD_OK;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_total, W.total, (size_t)Gp * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VROD_OK;
}
// Pass 2, behind pass 1 over the same table: the rows of every label with a segment offset (not kNoSegment) written to
// idx->lab_lists from that offset on, ascending; list_n rows in all.
static int label_scatter_pass(vrod_index* idx, hipStream_t s, const LabelPassWs& W, const uint32_t* h_seg_off, uint32_t Gp, uint64_t list_n) {
    VROD_TRY(idx->lab_lists.ensure(std::max<uint64_t>(list_n, 1) * 4));
    HIP_TRY(hipMemcpyAsync(W.seg_off, h_seg_off, (size_t)Gp * 4, hipMemcpyHostToDevice, s));
    if (list_n)
        launch_label_group_scatter(idx->labels.d(), idx->row_mask(), idx->count, W.rpb, W.table, Gp, W.cnt, Gp, W.seg_off,
                                   idx->lab_lists.as<uint32_t>(), s);
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}

// Device copies of a pass's slot tables (label_plan.h SlotTables): [slot_q | slot_len | slot_base], n words each.
struct DevSlots { uint32_t* q; uint32_t* len; uint32_t* base; };
static DevSlots dev_slots(uint32_t* p, size_t n) { return {p, p + n, p + 2 * n}; }

// The segmented route of one pass: the groups of T over the row lists in idx->lab_lists (enqueued on the slot's stream
// already), scored against the prepared queries d_q.  The tables go to D (slot_base only where the pass has one), then
// per chunk of the score block ONE score launch into P.scores -- between markers when `tm` is given -- and
// step(chunk, out_ld), which enqueues what reads the chunk's scores.  Returns with the stream drained.
template <typename Step>
static int run_segments(vrod_index* idx, Pending& P, Timer* tm, vrod_search_stats& st, const float* d_q, const SlotTables& T, const DevSlots& D,
                        Step&& step) {
    hipStream_t s = P.stream;
    const uint32_t ns = T.size();
    const SegPlan plan = plan_segments(T.segs);
    VROD_TRY(idx->lab_entries.ensure(std::max<size_t>(plan.entries.size(), 1) * sizeof(SegEntry)));
    HIP_TRY(hipMemcpyAsync(D.q, T.slot_q.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(D.len, T.slot_len.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
    if (!T.slot_base.empty()) HIP_TRY(hipMemcpyAsync(D.base, T.slot_base.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
    if (!plan.entries.empty())
        HIP_TRY(hipMemcpyAsync(idx->lab_entries.p, plan.entries.data(), plan.entries.size() * sizeof(SegEntry), hipMemcpyHostToDevice, s));
    for (const SegChunk& c : plan.chunks) {
        const uint64_t out_ld = round_up(std::max<uint32_t>(c.max_m, 1), 64);
        VROD_TRY(P.scores.ensure((size_t)c.n_slots * out_ld * 4));
        if (c.n_blocks) {
            size_t a = 0, b = 0;
            if (tm) VROD_TRY(tm->begin_launch(a, b));
            launch_rescore_segments(idx->corpus.p, idx->dtype, score_form(idx->metric), idx->dim, idx->ld, d_q, idx->lab_entries.as<SegEntry>() + c.e0,
                                    c.e1 - c.e0, c.n_blocks, D.q, c.slot0, idx->lab_lists.as<uint32_t>(), P.scores.as<float>(), out_ld, s);
            if (tm) VROD_TRY(tm->end_launch(a, b));
            st.scan_launches++;
        }
        VROD_TRY(step(c, out_ld));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s));   // the next pass reuses the tables
    return VROD_OK;
}

// ... of a labelled or tagged search: the select chain with a length per slot, then the k best of every slot to its
// query's result row.
static int score_segments(vrod_index* idx, Pending& P, Timer& tm, vrod_search_stats& st, const SlotTables& T, const DevSlots& D, uint32_t k,
                          uint64_t* d_out_ids, float* d_out_scores) {
    return run_segments(idx, P, &tm, st, P.q_f32.as<float>(), T, D, [&](const SegChunk& c, uint64_t out_ld) -> int {
        const uint64_t n_sel = std::max<uint32_t>(c.max_m, 1);
        const uint32_t kx = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, n_sel), kSelectChunk / 2);   // (the rest: unfilled)
        const uint64_t* keys; uint64_t kld, kn;
        VROD_TRY(select_chain(idx, P, P.scores.as<float>(), out_ld, n_sel, (int)c.n_slots, kx, nullptr, &keys, &kld, &kn, D.len + c.slot0));
        launch_seg_keys_to_output(keys, kld, kn, (int)c.n_slots, score_form(idx->metric), k, idx->lab_lists.as<uint32_t>(), D.base + c.slot0,
                                  D.q + c.slot0, idmap_of(idx), d_out_ids, d_out_scores, P.stream);
        return VROD_OK;
    });
}

// The workspace of the wide groups' searches: a group's mask, and the raw queries and results of up to max_nq queries.
static int wide_group_ws(vrod_index* idx, uint32_t max_nq, uint32_t k) {
    VROD_TRY(idx->lab_mask.ensure(idx->del_bits.size() * 4));   // capacity / 32 words
    VROD_TRY(idx->lab_q.ensure((size_t)max_nq * idx->dim * 4));
    return grow_lists(idx, 0, (size_t)max_nq * k);
}

// The dense route of one group: the ordinary search flow over the batch's queries d_qidx[0 .. nqg) with the group's mask
// (idx->lab_mask, enqueued on `s` already; m rows are clear in it) in place of row_mask(), the results scattered to the
// queries' rows.  lab_q and set 0 of the shared lists hold nqg queries.
static int dense_group_search(vrod_index* idx, hipStream_t s, vrod_search_stats& st, const float* d_queries_raw, const uint32_t* d_qidx,
                              const uint32_t* d_ones, uint32_t nqg, uint64_t m, uint32_t k, uint64_t* d_out_ids, float* d_out_scores) {
    launch_gather_rows(d_queries_raw, d_qidx, nqg, idx->dim, idx->lab_q.as<float>(), s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    idx->mask_ovr = idx->lab_mask.as<uint32_t>();
    idx->elig_ovr = m;
    const int rc = run_search(idx, idx->lab_q.as<float>(), nqg, k, idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>());
    idx->mask_ovr = nullptr;
    idx->elig_ovr = 0;
    if (rc != VROD_OK) return rc;
    fold_stats(st, idx->stats);
    st.scan_bytes += (double)idx->count * idx->ld * idx->esize;
    st.scan_flops += 2.0 * nqg * (double)idx->count * idx->dim;
    launch_scatter_results(idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>(), d_qidx, d_ones, nqg, k, d_out_ids, d_out_scores, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return VROD_OK;
}

// ------------------------------------------------------------------ searches over groups of rows (vrod_search_labeled, _tagged, _where)
// What the flow below needs of a predicate type: its grouping, the groups one pass serves, the bytes the row lists of
// one scatter pass may take, and the three launches over the handle's side arrays -- count and scatter over a pass's
// table, and one predicate's effective mask.
struct LabelSearch {
    using Pred = uint32_t;
    static constexpr uint32_t kGroupsPerPass = kLabelGroupsPerPass;
    static constexpr uint64_t kMaxListBytes = kNoListLimit;   // a row carries one label: a chunk's lists hold the corpus at the most
    static LabelGroups groups(const uint32_t* p, uint32_t nq) { return label_groups(p, nq); }
    static void count(const vrod_index* idx, const uint32_t* mask, uint32_t rpb, const uint32_t* table, uint32_t G, uint32_t* cnt, uint32_t cnt_ld,
                      hipStream_t s) {
        launch_label_group_count(idx->labels.d(), mask, idx->count, rpb, table, G, cnt, cnt_ld, s);
    }
    static void scatter(const vrod_index* idx, const uint32_t* mask, uint32_t rpb, const uint32_t* table, uint32_t G, const uint32_t* cnt,
                        uint32_t cnt_ld, const uint32_t* seg_off, uint32_t* lists, hipStream_t s) {
        launch_label_group_scatter(idx->labels.d(), mask, idx->count, rpb, table, G, cnt, cnt_ld, seg_off, lists, s);
    }
    static void mask_of(const vrod_index* idx, const uint32_t* mask, uint64_t words, uint32_t label, uint32_t* out, hipStream_t s) {
        launch_label_group_mask(idx->labels.d(), mask, idx->count, words, label, out, s);
    }
};
// Tags, and tags + value: the kernels of kernels_pred.hip over the handle's columns of that kind of row.
template <typename Rows> static Rows rows_of(const vrod_index* idx);
template <> TagRows rows_of(const vrod_index* idx) { return {idx->tags.d()}; }
template <> WhereRows rows_of(const vrod_index* idx) { return {idx->tags.d(), idx->values.d()}; }
template <> RowPredRows rows_of(const vrod_index* idx) { return {idx->tags.d(), idx->values.d(), idx->labels.d()}; }
template <typename Rows, uint32_t PER_PASS>
struct ColumnSearch {
    using Pred = typename Rows::Pred;
    static constexpr uint32_t kGroupsPerPass = PER_PASS;
    static constexpr uint64_t kMaxListBytes = 1ull << 30;   // a row sits in every list it matches: the 1 GiB rule
    static void count(const vrod_index* idx, const uint32_t* mask, uint32_t rpb, const Pred* table, uint32_t G, uint32_t* cnt, uint32_t cnt_ld,
                      hipStream_t s) {
        launch_pred_group_count(rows_of<Rows>(idx), mask, idx->count, rpb, table, G, cnt, cnt_ld, s);
    }
    static void scatter(const vrod_index* idx, const uint32_t* mask, uint32_t rpb, const Pred* table, uint32_t G, const uint32_t* cnt,
                        uint32_t cnt_ld, const uint32_t* seg_off, uint32_t* lists, hipStream_t s) {
        launch_pred_group_scatter(rows_of<Rows>(idx), mask, idx->count, rpb, table, G, cnt, cnt_ld, seg_off, lists, s);
    }
    static void mask_of(const vrod_index* idx, const uint32_t* mask, uint64_t words, const Pred& p, uint32_t* out, hipStream_t s) {
        launch_pred_group_mask(rows_of<Rows>(idx), mask, idx->count, words, p, out, s);
    }
};
struct TagSearch : ColumnSearch<TagRows, kTagGroupsPerPass> {
    static TagGroups groups(const TagPred* p, uint32_t nq) { return tag_groups(p, nq); }
};
struct WhereSearch : ColumnSearch<WhereRows, kWhereGroupsPerPass> {
    static WhereGroups groups(const WherePred* p, uint32_t nq) { return where_groups(p, nq); }
};

// Query q sees the eligible rows (live, allowed) that match h_preds[q]: carry its label, match its tag predicate, or
// match its tags + value-interval predicate (label_plan.h, kernels_label.hip; tag_plan.h, where_plan.h,
// kernels_pred.hip).  A group is a distinct predicate.  Every chunk of S::kGroupsPerPass groups is counted first -- one
// pass over the side arrays, into a [blocks][groups] matrix -- and its groups routed by filter_route -- the rule of a
// filtered search, with the group's rows and queries -- to
//   the segmented route: the canonical scores of its own rows, all such groups of a scatter pass in one launch per
//     score chunk (kernels_rescore.hip rescore_segments_kernel), the select chain with a length per query, exact by
//     construction as the gather path is; or
//   the dense route: the ordinary search flow (fast pass, certificate, band, exact) over the whole corpus with the
//     group's mask -- handle mask | no match -- in place of row_mask(): broad groups are few, one search each.
// The chunk's narrow groups' row lists are written and scored in passes whose lists stay under S::kMaxListBytes (a row
// belongs to every tag or where group it matches, so their sum is not bounded by the corpus; labels' groups are
// disjoint and a chunk is one pass), each pass one segmented score launch per score chunk; after the last chunk the
// wide groups take one masked ordinary search each.  Queries whose predicate no row can match (all & none != 0, an
// empty interval) are in no group: their result rows are filled as unfilled and nothing else looks at them.
// Synchronous: the handle is idle before and after.  d_queries_raw / d_out_*: device memory, h_preds: host.
template <typename S>
static int pred_search(vrod_index* idx, const float* d_queries_raw, uint32_t nq, uint32_t k, const typename S::Pred* h_preds,
                       uint64_t* d_out_ids, float* d_out_scores) {
    using Pred = typename S::Pred;
    constexpr uint32_t kPerPass = S::kGroupsPerPass;
    vrod_search_stats st{};
    st.nq = nq; st.k = k; st.path = VROD_PATH_GATHER;
    const uint64_t N = idx->count;
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    if (N == 0) return return_unfilled(idx, s, st, d_out_ids, d_out_scores, (uint64_t)nq * k);   // an empty handle
    VROD_TRY(prep_queries_checked(idx, P, d_queries_raw, nq));

    const auto G = S::groups(h_preds, nq);   // PredGroups<Pred>
    const uint32_t Gn = G.size();
    if (!Gn) return return_unfilled(idx, s, st, d_out_ids, d_out_scores, (uint64_t)nq * k);   // no predicate can match
    if (G.n_unsatisfiable()) {   // (the groups' queries overwrite their own rows below)
        launch_fill_none(d_out_ids, d_out_scores, (uint64_t)nq * k, s);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t* base_mask = idx->row_mask();
    const uint32_t rpb = label_rows_per_block(N);
    const uint32_t n_blocks = (uint32_t)((N + rpb - 1) / rpb);
    const double row_bytes = (double)idx->ld * idx->esize;
    // device copy of q_order (a dense group's queries, and the scatter of its results) followed by as many ones, then the
    // per-slot arrays of the segmented route
    VROD_TRY(idx->lab_slots.ensure((size_t)nq * 4 * 5));
    uint32_t* d_qorder = idx->lab_slots.as<uint32_t>();
    uint32_t* d_ones = d_qorder + nq;
    const DevSlots d_slots = dev_slots(d_ones + nq, nq);
    // [predicates | totals | a pass's segment offsets] and the count matrix [blocks][groups] of ONE chunk of
    // kPerPass groups: the workspace does not grow with the batch's distinct predicates
    const uint32_t Gc = std::min(Gn, kPerPass);
    VROD_TRY(idx->lab_tab.ensure((size_t)Gc * (sizeof(Pred) + 8)));
    VROD_TRY(idx->lab_cnt.ensure((size_t)n_blocks * Gc * 4));
    Pred* d_table = idx->lab_tab.template as<Pred>();
    uint32_t* d_total = (uint32_t*)(d_table + Gc);
    uint32_t* d_seg_off = d_total + Gc;
    uint32_t* d_cnt = idx->lab_cnt.as<uint32_t>();
    std::vector<uint32_t> m(Gn);
    std::vector<uint8_t> narrow(Gn);
    {
        std::vector<uint32_t> up(G.q_order);
        up.resize((size_t)nq * 2, 1u);
        HIP_TRY(hipMemcpyAsync(d_qorder, up.data(), up.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    Timer tm(idx, P);
    P.reset_events();
    for (uint32_t c0 = 0; c0 < Gn; c0 += kPerPass) {
        const uint32_t Gp = std::min(kPerPass, Gn - c0);
        // ---- pass 1: the chunk's groups' eligible matching rows, counted per block of the side arrays
        HIP_TRY(hipMemcpyAsync(d_table, G.preds.data() + c0, (size_t)Gp * sizeof(Pred), hipMemcpyHostToDevice, s));
        S::count(idx, base_mask, rpb, d_table, Gp, d_cnt, Gp, s);
        launch_group_prefix(d_cnt, n_blocks, Gp, d_total, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(m.data() + c0, d_total, (size_t)Gp * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // ---- route
        for (uint32_t g = c0; g < c0 + Gp; ++g) narrow[g] = filter_route(idx->path, idx->dtype, N, m[g], G.nq_of(g), idx->dim);
        const std::vector<uint32_t> mc(m.begin() + c0, m.begin() + c0 + Gp);
        const std::vector<uint8_t> nc(narrow.begin() + c0, narrow.begin() + c0 + Gp);
        // ---- pass 2 per scatter pass: the narrow groups' row lists, ascending, then score + select
        for (const TagPass& tp : plan_tag_passes(mc, nc, S::kMaxListBytes, kPerPass)) {
            SlotTables T;
            for (uint32_t i = tp.g0; i < tp.g1; ++i) {
                const uint32_t g = c0 + i, base = tp.seg_off[i - tp.g0], nqg = G.nq_of(g);
                if (base == kNoSegment) continue;
                T.add(base, m[g], &G.q_order[G.q_off[g]], nqg);
                st.scan_bytes += (double)m[g] * row_bytes;
                st.scan_flops += 2.0 * nqg * (double)m[g] * idx->dim;
            }
            VROD_TRY(idx->lab_lists.ensure(std::max<uint64_t>(tp.list_n, 1) * 4));
            HIP_TRY(hipMemcpyAsync(d_seg_off, tp.seg_off.data(), (size_t)(tp.g1 - tp.g0) * 4, hipMemcpyHostToDevice, s));
            if (tp.list_n)
                S::scatter(idx, base_mask, rpb, d_table + tp.g0, tp.g1 - tp.g0, d_cnt + tp.g0, Gp, d_seg_off, idx->lab_lists.template as<uint32_t>(), s);
            HIP_TRY(hipGetLastError());
            VROD_TRY(score_segments(idx, P, tm, st, T, d_slots, k, d_out_ids, d_out_scores));
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    tm.add_scan_ms(st);

    // ---- wide groups: one ordinary search each, over the predicate's mask
    uint32_t max_nq = 0;
    for (uint32_t g = 0; g < Gn; ++g) if (!narrow[g]) max_nq = std::max(max_nq, G.nq_of(g));
    if (max_nq) {
        const uint64_t words = idx->del_bits.size();   // capacity / 32
        VROD_TRY(wide_group_ws(idx, max_nq, k));
        for (uint32_t g = 0; g < Gn; ++g) {
            if (narrow[g]) continue;
            S::mask_of(idx, base_mask, words, G.preds[g], idx->lab_mask.template as<uint32_t>(), s);
            VROD_TRY(dense_group_search(idx, s, st, d_queries_raw, d_qorder + G.q_off[g], d_ones, G.nq_of(g), m[g], k, d_out_ids, d_out_scores));
        }
    }
    idx->stats = st;
    return VROD_OK;
}

// ------------------------------------------------------------------ grouped search (vrod_search_grouped)
// The best eligible row of each label (its representative), the k best representatives per query.  A search's list is
// sorted by (score, id), so the representatives, in their own order, are a sub-sequence of it: the first k distinct
// labels of an exact top-k1 are the k best representatives whenever the list has that many, or holds every eligible row.
//   candidate stage: the ordinary search flow with k1 = group_first_k results per query (group_plan.h), then
//     group_dedupe_kernel keeps the first entry of each label (kernels_group.hip);
//   dense stage, for the queries that stage leaves unresolved (a few labels own their whole list) and for every query
//     under VROD_PATH_EXACT: the canonical scores of all rows, once per group of up to 8 queries, then rounds of
//     [mask per query: the handle's mask | rows of a label already taken -> select the next k1 -> de-duplicate] until the
//     query is resolved.  A round that does not resolve its query returns k1 unmasked rows, so it takes at least one new
//     label and masks all of that label's rows: at most k rounds.
// Synchronous: the handle is idle before and after.  Every pointer is device memory; d_out_labels is never null here.
static int grouped_search(vrod_index* idx, const float* d_queries_raw, uint32_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                          uint32_t* d_out_labels) {
    vrod_search_stats st{};
    st.nq = nq; st.k = k; st.path = (uint32_t)idx->path;
    const uint64_t N = idx->count, elig = idx->eligible();
    const int form = score_form(idx->metric);
    const IdMap idmap = idmap_of(idx);
    hipStream_t s = next_slot(idx).stream;
    VROD_TRY(idx->grp_small.ensure((size_t)nq * 4 * 3));
    uint32_t* d_found = idx->grp_small.as<uint32_t>();
    uint32_t* d_valid = d_found + nq;
    uint32_t* d_qidx = d_valid + nq;
    launch_fill_none(d_out_ids, d_out_scores, (uint64_t)nq * k, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(d_out_labels, 0, (size_t)nq * k * 4, s));
    HIP_TRY(hipMemsetAsync(d_found, 0, (size_t)nq * 4 * 2, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (N == 0 || elig == 0) {   // no eligible row: every slot unfilled, as vrod_search
        idx->stats = st;
        return VROD_OK;
    }
    // a handle without labels holds one label: its representative is the best row, and no list can add a second
    const bool one_label = !idx->labels.exists();
    const uint32_t k1 = one_label ? 1u : group_first_k(k, elig);
    std::vector<uint32_t> hfv((size_t)nq * 2), todo;
    auto read_state = [&](hipStream_t on) -> int {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(hfv.data(), d_found, (size_t)nq * 8, hipMemcpyDeviceToHost, on));
        HIP_TRY(hipStreamSynchronize(on));
        return VROD_OK;
    };
    auto resolved = [&](uint32_t q) { return one_label || group_resolved(hfv[q], k, hfv[nq + q], k1, elig); };

    // ---- candidate stage
    if (idx->path != VROD_PATH_EXACT) {
        VROD_TRY(grow_lists(idx, 0, (size_t)nq * k1));
        VROD_TRY(run_search(idx, d_queries_raw, nq, k1, idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>()));
        st = idx->stats;
        st.k = k;
        s = next_slot(idx).stream;
        launch_group_dedupe(idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>(), k1, nq, idx->labels.d(), idmap.offset, nullptr, k,
                            d_out_ids, d_out_scores, d_out_labels, d_found, d_valid, s);
        VROD_TRY(read_state(s));
        for (uint32_t q = 0; q < nq; ++q)
            if (!resolved(q)) todo.push_back(q);
    } else {
        for (uint32_t q = 0; q < nq; ++q) todo.push_back(q);
    }
    if (todo.empty()) {
        idx->stats = st;
        return VROD_OK;
    }

    // ---- dense stage: the queries prepared as a search prepares them (NaN / Inf fails the call: under EXACT nothing
    // has looked at them yet)
    Pending& P = next_slot(idx);
    VROD_TRY(prep_queries_checked(idx, P, d_queries_raw, nq));

    const uint64_t score_ld = round_up(N, 64), words = idx->del_bits.size();   // capacity / 32
    const double row_bytes = (double)idx->ld * idx->esize;
    int gmax = rescore_all_max_queries(idx->ld);
    while (gmax > 1 && (uint64_t)gmax * score_ld * 4 > (1ull << 30)) gmax >>= 1;
    VROD_TRY(grow_lists(idx, 0, (size_t)gmax * k1));   // (the candidate stage's lists are spent: their reader was drained)
    VROD_TRY(idx->grp_mask.ensure((size_t)gmax * words * 4));
    Timer tm(idx, P);
    P.reset_events();
    for (size_t f0 = 0; f0 < todo.size();) {
        int g = gmax;
        while ((size_t)g > todo.size() - f0) g >>= 1;
        VROD_TRY(P.scores.ensure((size_t)g * score_ld * 4));
        size_t ea = 0, eb = 0;
        VROD_TRY(tm.begin_launch(ea, eb));
        launch_rescore_all(idx->corpus.p, idx->dtype, form, idx->dim, idx->ld, P.q_f32.as<float>(), &todo[f0], g, N, P.scores.as<float>(),
                           score_ld, s);
        VROD_TRY(tm.end_launch(ea, eb));
        HIP_TRY(hipGetLastError());
        st.scan_launches++;
        st.scan_bytes += (double)N * row_bytes;
        st.scan_flops += 2.0 * g * (double)N * idx->dim;
        struct Active { uint32_t q, score_row; };
        std::vector<Active> act;
        for (int i = 0; i < g; ++i) act.push_back({todo[f0 + i], (uint32_t)i});
        for (uint32_t round = 0; !act.empty(); ++round) {
            if (round > k) return fail(VROD_ERR_INTERNAL, "grouped search: a dense round took no label");
            const uint32_t na = (uint32_t)act.size();
            std::vector<uint32_t> hq(na);
            for (uint32_t a = 0; a < na; ++a) hq[a] = act[a].q;
            HIP_TRY(hipMemcpyAsync(d_qidx, hq.data(), (size_t)na * 4, hipMemcpyHostToDevice, s));
            launch_group_mask(idx->labels.d(), idx->row_mask(), N, words, d_qidx, na, d_out_labels, d_found, k, idx->grp_mask.as<uint32_t>(), s);
            for (uint32_t a = 0; a < na; ++a) {   // a mask per query: a select chain per query
                const uint64_t* keys; uint64_t kld, kn;
                VROD_TRY(select_chain(idx, P, P.scores.as<float>() + (size_t)act[a].score_row * score_ld, score_ld, N, 1, k1,
                                      idx->grp_mask.as<uint32_t>() + (size_t)a * words, &keys, &kld, &kn));
                launch_keys_to_output(keys, kn, form, k1, idmap, idx->list_ids[0].as<uint64_t>() + (size_t)a * k1,
                                      idx->list_scores[0].as<float>() + (size_t)a * k1, s);
            }
            launch_group_dedupe(idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>(), k1, na, idx->labels.d(), idmap.offset, d_qidx, k,
                                d_out_ids, d_out_scores, d_out_labels, d_found, d_valid, s);
            VROD_TRY(read_state(s));   // (also orders the next round's upload of d_qidx behind this round's readers)
            std::vector<Active> next;
            for (const Active& a : act)
                if (!resolved(a.q)) next.push_back(a);
            act.swap(next);
        }
        f0 += g;
    }
    tm.add_scan_ms(st);   // (every round ended with a synchronisation: the events are complete)
    st.fallback_queries += (uint32_t)todo.size();
    if (todo.size() == nq) st.path = VROD_PATH_EXACT;
    idx->stats = st;
    return VROD_OK;
}

// ------------------------------------------------------------------ multi-vector search (vrod_search_multivec)
// A query is the vectors [lims[q], lims[q + 1]) of the call, a document the eligible rows of one label, and
//     S(q, L) = M(first, L) + ... + M(last, L)   (fp32, from +0, left to right),  M(t, L) = the best canonical score of
// vector t over the document's rows; the k best documents per query, ties by the smaller label.  Two routes:
//   candidate route (multivec_candidates): the ordinary certified search for every vector of a sub-batch with k1 results
//     each; a query's candidates are the labels in any of its lists, de-duplicated on the device; their rows are grouped
//     by label (the labelled search's passes), scored against the vectors of every query that holds the label as a
//     candidate in the segmented launch, reduced to M per score slot and to S per (query, candidate), and ranked by the
//     select chain.  The answer stands when multivec_plan.h's certificate holds;
//   dense route (multivec_dense), for every other query and for all of them under VROD_PATH_EXACT: the canonical scores
//     of every row against up to 8 vectors at a time, folded into best[vector][document] and added into S[document]
//     group after group -- so the table never holds more than 8 vectors whatever the query's length -- then the select
//     chain over the documents, with the documents that have no eligible row masked out.
// Synchronous: the handle is idle before and after.  d_raw and the outputs are device memory, h_lims host memory.
static int multivec_doc_index(vrod_index* idx) {
    if (idx->doc_valid) return VROD_OK;
    const uint64_t N = idx->count;
    std::vector<uint32_t> docs(1, 0u);
    if (idx->labels.exists()) {
        docs.assign(idx->labels.host.begin(), idx->labels.host.begin() + N);
        std::sort(docs.begin(), docs.end());
        docs.erase(std::unique(docs.begin(), docs.end()), docs.end());
        std::vector<uint32_t> rank(N);
        for (uint64_t r = 0; r < N; ++r)
            rank[r] = (uint32_t)(std::lower_bound(docs.begin(), docs.end(), idx->labels.host[r]) - docs.begin());
        VROD_TRY(idx->doc_rank.ensure(N * 4));
        HIP_TRY(hipMemcpy(idx->doc_rank.p, rank.data(), N * 4, hipMemcpyHostToDevice));
    }
    VROD_TRY(idx->doc_labels.ensure(docs.size() * 4));
    HIP_TRY(hipMemcpy(idx->doc_labels.p, docs.data(), docs.size() * 4, hipMemcpyHostToDevice));
    idx->n_docs = docs.size();
    idx->doc_valid = true;
    return VROD_OK;
}

// The select chain, then one more pass over its keys: [nq][kp] keys sorted best first, 0 = none.
static int select_sorted(vrod_index* idx, Pending& P, const float* d_scores, uint64_t score_ld, uint64_t n, int nq, uint32_t kp,
                         const uint32_t* mask, const uint32_t* len, const uint64_t** out_keys) {
    const uint64_t* keys; uint64_t kld, kn;
    VROD_TRY(select_chain(idx, P, d_scores, score_ld, n, nq, kp, mask, &keys, &kld, &kn, len));
    DevBuf& dst = keys == P.keys_a.as<uint64_t>() ? P.keys_b : P.keys_a;
    VROD_TRY(dst.ensure((size_t)nq * kp * 8));
    launch_select_from_keys(keys, kld, kn, nq, kp, dst.as<uint64_t>(), kp, P.stream);
    *out_keys = dst.as<uint64_t>();
    return VROD_OK;
}

// The dense route for the queries `todo` (indices of the call), whose result rows it writes whole.
static int multivec_dense(vrod_index* idx, vrod_search_stats& st, const uint32_t* lims, const std::vector<uint32_t>& todo, uint32_t k,
                          uint32_t* d_out_labels, float* d_out_scores, uint32_t* d_found) {
    if (todo.empty()) return VROD_OK;
    VROD_TRY(multivec_doc_index(idx));
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    const int form = score_form(idx->metric);
    const uint64_t N = idx->count, D = idx->n_docs, score_ld = round_up(N, 64), Dld = round_up(D, 64);
    const double row_bytes = (double)idx->ld * idx->esize;
    const uint32_t gmax = (uint32_t)rescore_all_max_queries(idx->ld);   // 8
    const uint32_t qg_max = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, (1ull << 30) / (Dld * 4)));
    const uint32_t kx = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, D), kSelectChunk / 2);   // (the rest: unfilled)
    VROD_TRY(P.scores.ensure((size_t)gmax * score_ld * 4));
    VROD_TRY(idx->mv_best.ensure((size_t)gmax * D * 4));
    VROD_TRY(idx->mv_absent.ensure(((size_t)D + 31) / 32 * 4 + 64));
    VROD_TRY(idx->mv_S.ensure((size_t)std::min<size_t>(qg_max, todo.size()) * Dld * 4));
    VROD_TRY(idx->mv_pairs.ensure((size_t)qg_max * 4));
    uint32_t* d_qidx = idx->mv_pairs.as<uint32_t>();
    const uint32_t* d_rank = idx->labels.exists() ? idx->doc_rank.as<uint32_t>() : nullptr;
    bool have_absent = false;
    for (size_t f0 = 0; f0 < todo.size(); f0 += qg_max) {
        const uint32_t qg = (uint32_t)std::min<size_t>(qg_max, todo.size() - f0);
        for (uint32_t i = 0; i < qg; ++i) {
            const uint32_t q = todo[f0 + i];
            for (uint32_t v0 = lims[q]; v0 < lims[q + 1]; v0 += gmax) {
                const uint32_t g = std::min(gmax, lims[q + 1] - v0);
                uint32_t gl = 1;   // the launch takes 1, 2, 4 or 8 vectors: the last one repeats up to that
                while (gl < g) gl <<= 1;
                uint32_t qi[8];
                for (uint32_t j = 0; j < gl; ++j) qi[j] = v0 + std::min(j, g - 1);
                launch_rescore_all(idx->corpus.p, idx->dtype, form, idx->dim, idx->ld, idx->mv_q.as<float>(), qi, (int)gl, N, P.scores.as<float>(),
                                   score_ld, s);
                HIP_TRY(hipMemsetAsync(idx->mv_best.p, 0, (size_t)g * D * 4, s));
                launch_multivec_fold(P.scores.as<float>(), score_ld, g, N, d_rank, idx->row_mask(), form, idx->mv_best.as<uint32_t>(), D, s);
                launch_multivec_sum(idx->mv_best.as<uint32_t>(), g, D, form, v0 == lims[q], idx->mv_S.as<float>() + (size_t)i * Dld,
                                    have_absent ? nullptr : idx->mv_absent.as<uint32_t>(), s);
                HIP_TRY(hipGetLastError());
                have_absent = true;   // (the same for every vector and every query: which documents have an eligible row)
                st.scan_launches++;
                st.scan_bytes += (double)N * row_bytes;
                st.scan_flops += 2.0 * g * (double)N * idx->dim;
            }
        }
        const uint64_t* keys;
        VROD_TRY(select_sorted(idx, P, idx->mv_S.as<float>(), Dld, D, (int)qg, kx, idx->mv_absent.as<uint32_t>(), nullptr, &keys));
        HIP_TRY(hipMemcpyAsync(d_qidx, &todo[f0], (size_t)qg * 4, hipMemcpyHostToDevice, s));
        launch_multivec_output(keys, kx, kx, qg, form, k, idx->doc_labels.as<uint32_t>(), nullptr, d_qidx, d_out_labels, d_out_scores, d_found,
                               nullptr, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));   // the next group reuses S and the query indices
    }
    return VROD_OK;
}

// The candidate route for the sub-batch of queries [q0, q1): the result rows of the queries it certifies are final, the
// others are appended to `dense`.
static int multivec_candidates(vrod_index* idx, vrod_search_stats& st, bool first_batch, const float* d_raw, const uint32_t* lims, uint32_t q0,
                               uint32_t q1, uint32_t k, uint32_t k1, uint32_t* d_out_labels, float* d_out_scores, uint32_t* d_found,
                               std::vector<uint32_t>& dense) {
    const uint32_t nqs = q1 - q0, vbase = lims[q0], V = lims[q1] - vbase;
    const uint64_t N = idx->count, elig = idx->eligible();
    const int form = score_form(idx->metric);
    const double row_bytes = (double)idx->ld * idx->esize;
    vrod_multivec_stats& ms = idx->mv_stats;
    // ---- the certified lists of every vector
    VROD_TRY(grow_lists(idx, 0, (size_t)V * k1));
    VROD_TRY(run_search(idx, d_raw + (size_t)vbase * idx->dim, V, k1, idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>()));
    if (first_batch) {
        st = idx->stats;
    } else {
        fold_stats(st, idx->stats);
        st.scan_bytes += idx->stats.scan_bytes;
        st.scan_flops += idx->stats.scan_flops;
    }
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;

    // ---- the distinct labels of each query's lists, its flags and U
    std::vector<MultivecQuery> mq(nqs);
    uint64_t tab_words = 0;
    for (uint32_t i = 0; i < nqs; ++i) {
        const uint32_t m = lims[q0 + i + 1] - lims[q0 + i], slots = multivec_table_slots(m * k1);
        uint32_t bits = 0;
        while ((1u << bits) < slots) ++bits;
        mq[i] = MultivecQuery{lims[q0 + i] - vbase, m, (lims[q0 + i] - vbase) * k1, (uint32_t)tab_words, slots, 32 - bits};
        tab_words += slots;
    }
    const size_t entries = (size_t)V * k1;
    VROD_TRY(idx->mv_ent.ensure(entries * 4));
    VROD_TRY(idx->mv_cand.ensure(entries * 4));
    VROD_TRY(idx->mv_tab.ensure(tab_words * 4));
    // per query: [MultivecQuery | count | flags | U | kth | table offset | query index | candidates]
    VROD_TRY(idx->mv_small.ensure((size_t)nqs * (sizeof(MultivecQuery) + 7 * 4)));
    MultivecQuery* d_mq = idx->mv_small.as<MultivecQuery>();
    uint32_t* d_count = (uint32_t*)(d_mq + nqs);
    uint32_t* d_flags = d_count + nqs;
    float* d_U = (float*)(d_flags + nqs);
    float* d_kth = d_U + nqs;
    uint32_t* d_tab_off = (uint32_t*)(d_kth + nqs);
    uint32_t* d_qidx = d_tab_off + nqs;
    uint32_t* d_len = d_qidx + nqs;
    HIP_TRY(hipMemcpyAsync(d_mq, mq.data(), (size_t)nqs * sizeof(MultivecQuery), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(idx->mv_tab.p, 0xFF, tab_words * 4, s));
    launch_multivec_candidates(idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>(), k1, idx->labels.d(), idmap_of(idx).offset, d_mq, nqs,
                               idx->mv_ent.as<uint32_t>(), idx->mv_tab.as<uint32_t>(), idx->mv_cand.as<uint32_t>(), d_count, d_flags, d_U, s);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> cf((size_t)nqs * 3), cand(entries);
    HIP_TRY(hipMemcpyAsync(cf.data(), d_count, (size_t)nqs * 12, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cand.data(), idx->mv_cand.p, entries * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t* h_count = cf.data();
    const uint32_t* h_flags = h_count + nqs;
    const float* h_U = (const float*)(h_flags + nqs);

    // ---- the candidates' eligible rows, counted per label (passes of kLabelGroupsPerPass labels)
    std::vector<uint8_t> alive(nqs, 1);
    std::vector<uint32_t> labs;
    for (uint32_t i = 0; i < nqs; ++i) {
        if (h_flags[i] & 2u) { alive[i] = 0; continue; }   // a NaN or infinite score in a list: the bound says nothing
        uint32_t* c = cand.data() + mq[i].ent_off;
        std::sort(c, c + h_count[i]);   // ascending: the select's tie-break by smaller column is by smaller label
        labs.insert(labs.end(), c, c + h_count[i]);
    }
    std::sort(labs.begin(), labs.end());
    labs.erase(std::unique(labs.begin(), labs.end()), labs.end());
    LabelPassWs W;
    VROD_TRY(label_pass_ws(idx, (uint32_t)std::min<size_t>(std::max<size_t>(labs.size(), 1), kLabelGroupsPerPass), W));
    std::vector<uint32_t> rows_of(labs.size());
    for (size_t g0 = 0; g0 < labs.size(); g0 += kLabelGroupsPerPass) {
        const uint32_t Gp = (uint32_t)std::min<size_t>(kLabelGroupsPerPass, labs.size() - g0);
        VROD_TRY(label_count_pass(idx, s, W, labs.data() + g0, Gp, rows_of.data() + g0));
    }
    auto lab_index = [&](uint32_t label) { return (size_t)(std::lower_bound(labs.begin(), labs.end(), label) - labs.begin()); };

    // ---- route: a query whose candidates own too many rows, or whose score slots no longer fit, goes dense
    uint64_t total_slots = 0;
    std::vector<uint32_t> live;   // sub-batch indices of the queries that stay
    for (uint32_t i = 0; i < nqs; ++i) {
        if (!alive[i]) continue;
        uint64_t cand_rows = 0;
        const uint32_t* c = cand.data() + mq[i].ent_off;
        for (uint32_t j = 0; j < h_count[i]; ++j) cand_rows += rows_of[lab_index(c[j])];
        const uint64_t slots = (uint64_t)h_count[i] * mq[i].m;
        if (multivec_candidates_too_broad(cand_rows, N) || total_slots + slots > kMultivecMaxSlots) { alive[i] = 0; continue; }
        total_slots += slots;
        live.push_back(i);
        ms.candidate_labels += h_count[i];
        ms.candidate_rows += cand_rows;
    }
    for (uint32_t i = 0; i < nqs; ++i)
        if (!alive[i]) dense.push_back(q0 + i);
    if (live.empty()) return VROD_OK;

    // ---- the labels the live queries use, each with its users (query, candidate column)
    struct User { uint32_t li, col; };
    std::vector<std::vector<User>> users(labs.size());
    for (uint32_t li = 0; li < live.size(); ++li) {
        const uint32_t i = live[li];
        const uint32_t* c = cand.data() + mq[i].ent_off;
        for (uint32_t j = 0; j < h_count[i]; ++j) users[lab_index(c[j])].push_back({li, j});
    }
    std::vector<uint32_t> used;   // indices into labs, ascending
    for (size_t g = 0; g < labs.size(); ++g)
        if (!users[g].empty()) used.push_back((uint32_t)g);
    std::vector<std::vector<uint32_t>> pair_slot(live.size());
    for (uint32_t li = 0; li < live.size(); ++li) pair_slot[li].resize(h_count[live[li]]);
    VROD_TRY(idx->mv_M.ensure(std::max<uint64_t>(total_slots, 1) * 4));

    // ---- per pass: the labels' row lists, the segmented score launch, M per score slot
    uint32_t slot_base = 0;
    for (size_t u0 = 0; u0 < used.size(); u0 += kLabelGroupsPerPass) {
        const uint32_t Gp = (uint32_t)std::min<size_t>(kLabelGroupsPerPass, used.size() - u0);
        std::vector<uint32_t> table(Gp), seg_off(Gp);
        SlotTables T;   // (a label's slots are every vector of every query that holds it: filled here, no slot_base)
        uint64_t list_n = 0;
        for (uint32_t g = 0; g < Gp; ++g) {
            const uint32_t lab_i = used[u0 + g], m_rows = rows_of[lab_i];
            table[g] = labs[lab_i];
            seg_off[g] = (uint32_t)list_n;
            const uint32_t slot0 = T.size();
            for (const User& u : users[lab_i]) {
                const uint32_t q = q0 + live[u.li];
                pair_slot[u.li][u.col] = slot_base + T.size();
                for (uint32_t v = lims[q]; v < lims[q + 1]; ++v) { T.slot_q.push_back(v); T.slot_len.push_back(m_rows); }
            }
            const uint32_t nsl = T.size() - slot0;
            T.segs.push_back({(uint32_t)list_n, m_rows, slot0, nsl});
            list_n += m_rows;   // (the labels' rows are disjoint: at most N in all)
            st.scan_bytes += (double)m_rows * row_bytes;
            st.scan_flops += 2.0 * nsl * (double)m_rows * idx->dim;
        }
        const uint32_t ns = T.size();
        VROD_TRY(label_count_pass(idx, s, W, table.data(), Gp, nullptr));
        VROD_TRY(label_scatter_pass(idx, s, W, seg_off.data(), Gp, list_n));
        VROD_TRY(idx->lab_slots.ensure((size_t)ns * 4 * 2));
        const DevSlots D = dev_slots(idx->lab_slots.as<uint32_t>(), ns);
        // (no markers: this route's launches are not part of scan_ms)
        VROD_TRY(run_segments(idx, P, nullptr, st, idx->mv_q.as<float>(), T, D, [&](const SegChunk& c, uint64_t out_ld) -> int {
            launch_multivec_slot_best(P.scores.as<float>(), out_ld, c.n_slots, D.len + c.slot0, form, idx->mv_M.as<float>() + slot_base + c.slot0, s);
            return VROD_OK;
        }));
        slot_base += ns;
    }

    // ---- S per (query, candidate), the select chain with a length per query, the outputs, the certificate
    uint32_t max_c = 1;
    for (uint32_t i : live) max_c = std::max(max_c, h_count[i]);
    const uint64_t Sld = round_up(max_c, 64);
    const uint32_t rows_max = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(live.size(), (1ull << 30) / (Sld * 4)));
    VROD_TRY(idx->mv_S.ensure((size_t)rows_max * Sld * 4));
    HIP_TRY(hipMemcpyAsync(idx->mv_cand.p, cand.data(), entries * 4, hipMemcpyHostToDevice, s));   // (sorted per query now)
    for (size_t l0 = 0; l0 < live.size(); l0 += rows_max) {
        const uint32_t nr = (uint32_t)std::min<size_t>(rows_max, live.size() - l0);
        std::vector<uint32_t> p_slot, p_m, tab_off(nr), qidx(nr), len(nr);
        std::vector<uint64_t> p_dst;
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t li = (uint32_t)l0 + r, i = live[li];
            tab_off[r] = mq[i].ent_off; qidx[r] = q0 + i; len[r] = h_count[i];
            for (uint32_t j = 0; j < h_count[i]; ++j) {
                p_slot.push_back(pair_slot[li][j]); p_m.push_back(mq[i].m); p_dst.push_back((uint64_t)r * Sld + j);
            }
        }
        const uint32_t np = (uint32_t)p_slot.size();
        VROD_TRY(idx->mv_pairs.ensure((size_t)np * 16 + 64));
        uint64_t* d_dst = idx->mv_pairs.as<uint64_t>();
        uint32_t* d_pslot = (uint32_t*)(d_dst + np);
        uint32_t* d_pm = d_pslot + np;
        HIP_TRY(hipMemcpyAsync(d_dst, p_dst.data(), (size_t)np * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pslot, p_slot.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_pm, p_m.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_tab_off, tab_off.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_qidx, qidx.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_len, len.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
        launch_multivec_pair_sum(idx->mv_M.as<float>(), d_pslot, d_pm, d_dst, np, idx->mv_S.as<float>(), s);
        const uint32_t kx = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, max_c), kSelectChunk / 2);
        const uint64_t* keys;
        VROD_TRY(select_sorted(idx, P, idx->mv_S.as<float>(), Sld, max_c, (int)nr, kx, nullptr, d_len, &keys));
        launch_multivec_output(keys, kx, kx, nr, form, k, idx->mv_cand.as<uint32_t>(), d_tab_off, d_qidx, d_out_labels, d_out_scores, d_found,
                               d_kth, s);
        HIP_TRY(hipGetLastError());
        std::vector<float> kth(nr);
        HIP_TRY(hipMemcpyAsync(kth.data(), d_kth, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t i = live[l0 + r];
            const bool complete = multivec_lists_complete(h_flags[i] & 1u, k1, elig);
            if (multivec_certified(complete, h_count[i], k, kth[r], h_U[i], form == M_COSINE)) ms.certified_queries++;
            else dense.push_back(q0 + i);   // (its row is written again, whole, by the dense route)
        }
    }
    return VROD_OK;
}

static int multivec_search(vrod_index* idx, const float* d_raw, const uint32_t* lims, uint32_t nq, uint32_t k, uint32_t* d_out_labels,
                           float* d_out_scores, uint32_t* d_found) {
    vrod_search_stats st{};
    st.nq = nq; st.k = k; st.path = (uint32_t)idx->path;
    vrod_multivec_stats& ms = idx->mv_stats;
    ms = vrod_multivec_stats{};
    ms.nq = nq; ms.vectors = lims[nq];
    const uint64_t N = idx->count, elig = idx->eligible();
    hipStream_t s = next_slot(idx).stream;
    if (N == 0 || elig == 0) {   // no eligible row: every slot unfilled, the vectors are not looked at (as vrod_search)
        std::vector<uint32_t> nan((size_t)nq * k, kScoreNoneBits);
        HIP_TRY(hipMemcpyAsync(d_out_scores, nan.data(), nan.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(d_out_labels, 0, (size_t)nq * k * 4, s));
        HIP_TRY(hipMemsetAsync(d_found, 0, (size_t)nq * 4, s));
        HIP_TRY(hipStreamSynchronize(s));
        idx->stats = st;
        return VROD_OK;
    }
    // every vector prepared as a search prepares a query, and checked, before anything is written
    {
        Pending& P = next_slot(idx);
        VROD_TRY(prep_queries_checked(idx, P, d_raw, lims[nq]));
        VROD_TRY(idx->mv_q.ensure((size_t)lims[nq] * idx->ld * 4));
        HIP_TRY(hipMemcpyAsync(idx->mv_q.p, P.q_f32.p, (size_t)lims[nq] * idx->ld * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    std::vector<uint32_t> dense;
    // a handle without labels is one document that owns every row: nothing for the candidate route to narrow
    if (idx->path != VROD_PATH_EXACT && idx->labels.exists()) {
        const uint32_t k1 = multivec_first_k(k, elig);
        ms.k1 = k1;
        for (uint32_t q0 = 0; q0 < nq;) {
            const uint32_t q1 = multivec_cut(lims, nq, q0);
            VROD_TRY(multivec_candidates(idx, st, q0 == 0, d_raw, lims, q0, q1, k, k1, d_out_labels, d_out_scores, d_found, dense));
            q0 = q1;
        }
        st.nq = nq; st.k = k;
        std::sort(dense.begin(), dense.end());
    } else {
        for (uint32_t q = 0; q < nq; ++q) dense.push_back(q);
    }
    VROD_TRY(multivec_dense(idx, st, lims, dense, k, d_out_labels, d_out_scores, d_found));
    ms.dense_queries = (uint32_t)dense.size();
    st.fallback_queries += (uint32_t)dense.size();
    if (dense.size() == nq) st.path = VROD_PATH_EXACT;
    idx->stats = st;
    return VROD_OK;
}

// ------------------------------------------------------------------ diversified search (vrod_search_diverse)
// The ordinary certified search with `pool` results per query into the handle's lists, then ONE launch of the selection
// kernel (kernels_diverse.hip): a work-group per query picks min(k, filled) rows of its list by exact greedy MMR.  The
// first stage refuses NaN / Inf queries before anything is written; the outputs are written by the selection alone.
// Synchronous: the handle is idle before and after.  Every pointer is device memory; d_out_mmr may be null.
static int diverse_search(vrod_index* idx, const float* d_queries_raw, uint32_t nq, uint32_t k, uint32_t pool, float lambda,
                          uint64_t* d_out_ids, float* d_out_scores, float* d_out_mmr) {
    if (idx->count == 0 || idx->eligible() == 0) {   // no eligible row: every slot unfilled, the queries are not looked at
        vrod_search_stats st{};
        st.nq = nq; st.k = k; st.path = (uint32_t)idx->path;
        hipStream_t s = next_slot(idx).stream;
        if (d_out_mmr) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_out_mmr, (int)kScoreNoneBits, (size_t)nq * k, s));
        return return_unfilled(idx, s, st, d_out_ids, d_out_scores, (uint64_t)nq * k);
    }
    if (!diverse_waves(idx->dim, pool)) return fail(VROD_ERR_INTERNAL, "diversified search: no work-group fits dim %u, pool %u", idx->dim, pool);
    VROD_TRY(grow_lists(idx, 0, (size_t)nq * pool));
    VROD_TRY(run_search(idx, d_queries_raw, nq, pool, idx->list_ids[0].as<uint64_t>(), idx->list_scores[0].as<float>()));
    idx->stats.k = k;
    hipStream_t s = next_slot(idx).stream;
    launch_diverse_select(idx->corpus.p, idx->dtype, score_form(idx->metric), idx->dim, idx->ld, idx->list_ids[0].as<uint64_t>(),
                          idx->list_scores[0].as<float>(), nq, pool, k, lambda, idmap_of(idx).offset, d_out_ids, d_out_scores, d_out_mmr, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return VROD_OK;
}

// ------------------------------------------------------------------ searches by stored row (vrod_search_by_ids, vrod_knn_graph)
// The queries are rows the handle already holds: byid_gather_kernel copies them out of the corpus as fp32 (kernels_byid.hip)
// and the ordinary search flow takes them as given (prep_ovr) -- the stored row is the query bit for bit, so the scores
// are scores between stored rows and an L2 row is at distance +0.0 from itself.  With the self drop the search returns
// k + 1 results into the library's own lists and byid_drop_self_kernel writes the caller's k: the top k of S \ {self} is
// the top (k + 1) of S with self removed, whatever position self took (an exact duplicate with a smaller id ranks
// before it; under IP, or under a filter that leaves it out, it may not be in the list at all).
constexpr uint32_t kByidFlag = 16;   // word of idx->flags.p the gather raises for an id that is no live row

static int byid_search_begin(vrod_index* idx, const float* d_rows_f32, uint32_t nq, uint32_t k1, uint64_t* d_ids, float* d_scores) {
    idx->prep_ovr = M_L2;   // set for exactly the enqueue: nothing else prepares queries
    const int rc = search_begin(idx, d_rows_f32, nq, k1, d_ids, d_scores);
    idx->prep_ovr = -1;
    return rc;
}

// d_ids, d_out_*: device memory.  checked: the host has validated the ids already (the host form); else the gather does,
// and its flag is read before the search is begun: a failed call leaves the handle and the outputs as they were.
static int byid_search(vrod_index* idx, const uint64_t* d_ids, bool checked, uint32_t nq, uint32_t k, bool exclude_self,
                       uint64_t* d_out_ids, float* d_out_scores) {
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    const uint32_t k1 = byid_search_k(k, exclude_self);
    const bool staged = exclude_self;   // the search writes the library's lists, the drop launch the caller's rows
    uint64_t* l_ids = d_out_ids;
    float* l_scores = d_out_scores;
    if (staged) {
        VROD_TRY(grow_lists(idx, 0, (size_t)nq * k1));
        l_ids = idx->list_ids[0].as<uint64_t>();
        l_scores = idx->list_scores[0].as<float>();
    }
    VROD_TRY(P.q_raw.ensure((size_t)nq * idx->dim * 4));
    launch_byid_gather(idx->corpus.p, idx->dtype, idx->ld, idx->dim, idx->count, idx->id_offset, idx->n_deleted ? idx->del_dev.p : nullptr, d_ids,
                       nullptr, 0, nq, P.q_raw.as<float>(), checked ? nullptr : &idx->flags.p[kByidFlag], s);
    HIP_TRY(hipGetLastError());
    if (!checked) {   // (the search is begun only behind this read-back: a bad id leaves the caller's buffers untouched)
        uint32_t bad;
        VROD_TRY(take_flag(idx, kByidFlag, s, &bad));
        if (bad)
            return fail(VROD_ERR_INVALID_ARG, "an id is not a live row of this handle (ids %llu..%llu, deleted rows excluded)",
                        (unsigned long long)idx->id_offset, (unsigned long long)(idx->id_offset + idx->count));
    }
    VROD_TRY(byid_search_begin(idx, P.q_raw.as<float>(), nq, k1, l_ids, l_scores));
    VROD_TRY(search_end(idx));
    idx->stats.k = k;
    if (staged) {   // (the search is complete: any stream may follow it)
        launch_byid_drop_self(l_ids, l_scores, k1, nullptr, d_ids, 0, nq, k, d_out_ids, d_out_scores, idx->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(idx->stream));
    }
    return VROD_OK;
}

// ------------------------------------------------------------------ search by weighted examples (vrod_search_combined)
// The query is built on the device (combine_queries_kernel, kernels_combine.hip): the caller's vector, prepared as a search
// prepares a query, then the named stored rows as stored, each times its weight, added in the caller's order with two
// roundings per step.  The combined vector is an ordinary raw query: the search flow prepares it again (no prep_ovr).  A
// batch in which some query excludes ids runs the search with k1 = k + the largest excluded count into the library's own
// lists, and drop_excluded_kernel writes the caller's k; a batch that excludes nothing searches straight into the
// caller's rows.  Every pointer is device memory except the two lims arrays, which the host has validated (counts).
// checked: the host has validated the term ids and the weights as well; else the combine launch does.  Its flag word --
// the overflow check in either case -- is read before the search is begun: a refused call leaves the outputs as they were.
constexpr uint32_t kCombineFlag = 17;   // word of idx->flags.p the combine launch raises

struct CombineArgs {
    const float* d_vectors;        // raw [nq][dim], or null
    const float* d_vector_weights; // [nq], or null
    const uint32_t* d_term_lims;
    const uint64_t* d_term_ids;
    const float* d_term_weights;
    const uint32_t* d_excl_lims;   // null: no exclude list
    const uint64_t* d_excl_ids;
};

static int combined_search(vrod_index* idx, const CombineArgs& a, const CombineCounts& counts, uint32_t nq, uint32_t k, uint32_t flags,
                           uint64_t* d_out_ids, float* d_out_scores) {
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    const uint32_t k1 = combine_search_k(k, counts.max_excluded);
    const bool staged = counts.max_excluded != 0;   // the search writes the library's lists, the drop launch the caller's rows
    uint64_t* l_ids = d_out_ids;
    float* l_scores = d_out_scores;
    if (staged) {
        VROD_TRY(grow_lists(idx, 0, (size_t)nq * k1));
        l_ids = idx->list_ids[0].as<uint64_t>();
        l_scores = idx->list_scores[0].as<float>();
    }
    if (a.d_vectors) VROD_TRY(prep_queries_checked(idx, P, a.d_vectors, nq));   // -> P.q_f32 [nq][ld]; NaN / Inf fails here
    VROD_TRY(P.q_raw.ensure((size_t)nq * idx->dim * 4));
    launch_combine_queries(idx->corpus.p, idx->dtype, idx->ld, idx->dim, idx->count, idx->id_offset, idx->n_deleted ? idx->del_dev.p : nullptr,
                           a.d_vectors ? P.q_f32.as<float>() : nullptr, a.d_vector_weights, a.d_term_lims, a.d_term_ids, a.d_term_weights, nq,
                           P.q_raw.as<float>(), &idx->flags.p[kCombineFlag], s);
    HIP_TRY(hipGetLastError());
    uint32_t bad;
    VROD_TRY(take_flag(idx, kCombineFlag, s, &bad));
    if (bad) {
        if (bad & kCombineBadId)
            return fail(VROD_ERR_INVALID_ARG, "a term id is not a live row of this handle (ids %llu..%llu, deleted rows excluded)",
                        (unsigned long long)idx->id_offset, (unsigned long long)(idx->id_offset + idx->count));
        if (bad & kCombineBadWeight) return fail(VROD_ERR_INVALID_VALUE, "a weight is NaN or Inf");
        return fail(VROD_ERR_INVALID_VALUE, "a combined vector holds NaN or Inf (overflow)");
    }
    VROD_TRY(run_search(idx, P.q_raw.as<float>(), nq, k1, l_ids, l_scores));
    idx->stats.k = k;
    if (staged) {   // (the search is complete: any stream may follow it)
        const bool with_terms = flags & VROD_COMBINED_EXCLUDE_TERMS;
        launch_drop_excluded(l_ids, l_scores, k1, a.d_excl_lims, a.d_excl_ids, with_terms ? a.d_term_lims : nullptr, a.d_term_ids, nq, k, d_out_ids,
                             d_out_scores, idx->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(idx->stream));
    }
    return VROD_OK;
}

// ------------------------------------------------------------------ candidate-list searches (vrod_search_candidates, vrod_score_candidates)
// Query q sees the rows its own list of ids names: the distinct ids that are current rows, live and allowed.  The lists
// are resolved on the device (kernels_candidates.hip) -- ids to local rows against row_mask(), the mask every search
// reads -- so neither form copies an id to the host.
//   the search form sorts every resolved list ascending and drops repeats (one work-group per query, launches by sort
//     class: candidates_plan.h), reads the nq lengths back and hands the segmented driver one group of one slot per
//     query: the canonical scores of its own rows, the select chain with a length per slot, exact by construction as a
//     labelled search's segmented route is.  There is no fast pass, no certificate and no route to choose;
//   the score form walks the canonical chain of every entry of the resolved, unsorted lists in ONE launch, one (query,
//     entry) pair per lane, and writes each score at its entry's position.
// Synchronous: the handle is idle before and after.  Every pointer is device memory except h_lims, which the host has
// validated (cand_check_lims); d_lims is its device copy.
static_assert(kCandMaxList == VROD_MAX_CANDIDATES, "candidates_plan.h restates VROD_MAX_CANDIDATES");

static int candidates_resolve(vrod_index* idx, hipStream_t s, const uint64_t* d_ids, uint32_t n) {
    VROD_TRY(idx->cand_rows.ensure((size_t)n * 4));
    launch_cand_resolve(d_ids, n, idx->count, idx->id_offset, idx->row_mask(), idx->cand_rows.as<uint32_t>(), s);
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}

static int candidates_search(vrod_index* idx, const float* d_queries_raw, uint32_t nq, uint32_t k, const uint32_t* h_lims, const uint32_t* d_lims,
                             const uint64_t* d_ids, uint64_t* d_out_ids, float* d_out_scores) {
    vrod_search_stats st{};
    st.nq = nq; st.k = k; st.path = VROD_PATH_GATHER;
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    const uint64_t nk = (uint64_t)nq * k;
    if (idx->count == 0 || idx->eligible() == 0) return return_unfilled(idx, s, st, d_out_ids, d_out_scores, nk);   // no row can answer
    VROD_TRY(prep_queries_checked(idx, P, d_queries_raw, nq));
    const uint32_t n_entries = h_lims[nq];
    if (!n_entries) return return_unfilled(idx, s, st, d_out_ids, d_out_scores, nk);   // every list is empty

    // ---- ids -> rows, then per query the ascending distinct rows into its segment of lab_lists, and their number
    VROD_TRY(candidates_resolve(idx, s, d_ids, n_entries));
    VROD_TRY(idx->lab_lists.ensure((size_t)n_entries * 4));
    VROD_TRY(idx->cand_small.ensure((size_t)nq * 4 * 2));
    uint32_t* d_len = idx->cand_small.as<uint32_t>();
    uint32_t* d_order = d_len + nq;
    const CandSortPlan sp = cand_sort_plan(h_lims, nq);
    HIP_TRY(hipMemcpyAsync(d_order, sp.order.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
    for (uint32_t c = 0; c < kCandClasses; ++c)
        launch_cand_sort_unique(idx->cand_rows.as<uint32_t>(), d_lims, d_order + sp.first[c], sp.first[c + 1] - sp.first[c], c,
                                idx->lab_lists.as<uint32_t>(), d_len, s);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> len(nq);
    HIP_TRY(hipMemcpyAsync(len.data(), d_len, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    // ---- one slot and one segment per query that has a row; the others' result rows are unfilled
    const CandSlots S = cand_slot_tables(h_lims, len.data(), nq);
    st.kprime = S.max_len;
    st.scan_bytes = (double)S.rows * idx->ld * idx->esize;
    st.scan_flops = 2.0 * (double)S.rows * idx->dim;
    if (S.n_empty) {   // (the other queries overwrite their own rows below)
        launch_fill_none(d_out_ids, d_out_scores, nk, s);
        HIP_TRY(hipGetLastError());
    }
    if (S.T.size()) {
        VROD_TRY(idx->lab_slots.ensure((size_t)S.T.size() * 4 * 3));
        const DevSlots d_slots = dev_slots(idx->lab_slots.as<uint32_t>(), S.T.size());
        Timer tm(idx, P);
        P.reset_events();
        VROD_TRY(score_segments(idx, P, tm, st, S.T, d_slots, k, d_out_ids, d_out_scores));
        tm.add_scan_ms(st);
    }
    HIP_TRY(hipStreamSynchronize(s));
    idx->stats = st;
    return VROD_OK;
}

static int candidates_score(vrod_index* idx, const float* d_queries_raw, uint32_t nq, const uint32_t* h_lims, const uint32_t* d_lims,
                            const uint64_t* d_ids, float* d_out_scores) {
    vrod_search_stats st{};
    st.nq = nq; st.k = 0; st.path = VROD_PATH_GATHER;
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    const uint32_t n_entries = h_lims[nq];
    if (idx->count == 0 || idx->eligible() == 0) {   // no row can be scored: every entry is ignored
        if (n_entries) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_out_scores, (int)kScoreNoneBits, n_entries, s));
        HIP_TRY(hipStreamSynchronize(s));
        idx->stats = st;
        return VROD_OK;
    }
    VROD_TRY(prep_queries_checked(idx, P, d_queries_raw, nq));
    if (n_entries) {
        VROD_TRY(candidates_resolve(idx, s, d_ids, n_entries));
        // [entries scored per query | the tile offsets of the launch]
        const std::vector<uint32_t> off = cand_tile_offsets(h_lims, nq);
        VROD_TRY(idx->cand_small.ensure(((size_t)nq * 2 + 1) * 4));
        uint32_t* d_cnt = idx->cand_small.as<uint32_t>();
        uint32_t* d_off = d_cnt + nq;
        HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t)nq * 4, s));
        HIP_TRY(hipMemcpyAsync(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
        Timer tm(idx, P);
        P.reset_events();
        size_t a = 0, b = 0;
        VROD_TRY(tm.begin_launch(a, b));
        launch_cand_score(idx->corpus.p, idx->dtype, score_form(idx->metric), idx->dim, idx->ld, P.q_f32.as<float>(), d_lims, d_off, nq, off[nq],
                          idx->cand_rows.as<uint32_t>(), d_out_scores, d_cnt, s);
        VROD_TRY(tm.end_launch(a, b));
        HIP_TRY(hipGetLastError());
        st.scan_launches = 1;
        std::vector<uint32_t> cnt(nq);
        HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        tm.add_scan_ms(st);
        uint64_t rows = 0;   // entries scored: a repeated id is scored at every position
        for (uint32_t q = 0; q < nq; ++q) { rows += cnt[q]; st.kprime = std::max(st.kprime, cnt[q]); }
        st.scan_bytes = (double)rows * idx->ld * idx->esize;
        st.scan_flops = 2.0 * (double)rows * idx->dim;
    }
    idx->stats = st;
    return VROD_OK;
}

// The graph of rows [row0, row0 + n): batches of byid_plan.h, two in flight -- batch s + 1's gather and search are
// enqueued (search_begin) before batch s is completed (search_end), its lists lose self and its rows are copied out, so
// the device scans batch s + 1 while the host and the copy engine finish batch s.  The deleted rows of a batch never
// reach the scan: byid_live_kernel compacts the batch's live rows (their number comes from the host mirror), and the
// drop launch writes the deleted rows' result rows unfilled.  out_*: host memory.
static int knn_graph(vrod_index* idx, uint64_t row0, uint64_t n, uint32_t k, uint64_t* out_ids, float* out_scores) {
    const uint32_t k1 = byid_search_k(k, true);
    const uint32_t batch = byid_batch_rows(idx->dtype == VROD_DTYPE_BF16, n);
    const uint64_t nb = byid_n_batches(n, batch);
    vrod_search_stats tot{};
    tot.k = k; tot.path = (uint32_t)idx->path;
    struct Flight { ByidBatch b; uint32_t live; bool holes; hipStream_t stream; };
    auto map_of = [&](const Flight& F) { return idx->byid_map[F.b.slot].as<uint32_t>(); };   // [live rows | place of every row]
    auto begin = [&](uint64_t s, Flight& F) -> int {
        F.b = byid_batch(n, batch, s);
        const uint64_t r0 = row0 + F.b.first;
        const uint32_t m = F.b.rows, c = F.b.slot;
        uint32_t dead = 0;
        if (idx->n_deleted) {   // the tombstones of [r0, r0 + m), a word of the host mirror at a time
            const uint32_t* bits = idx->del_bits.data();
            for (uint64_t w = r0 / 32; w * 32 < r0 + m; ++w) {
                uint32_t v = bits[w];
                if (w * 32 < r0) v &= ~0u << (r0 - w * 32);
                if ((w + 1) * 32 > r0 + m) v &= ~0u >> ((w + 1) * 32 - (r0 + m));
                dead += (uint32_t)__builtin_popcount(v);
            }
        }
        F.live = m - dead;
        F.holes = dead != 0;
        F.stream = idx->stream;
        if (!F.live) return VROD_OK;   // nothing to search: the batch's rows are written unfilled
        Pending& P = next_slot(idx);
        F.stream = P.stream;
        VROD_TRY(grow_lists(idx, (int)c, (size_t)F.live * k1));
        VROD_TRY(P.q_raw.ensure((size_t)F.live * idx->dim * 4));
        const uint32_t* d_rows = nullptr;
        if (F.holes) {
            VROD_TRY(idx->byid_map[c].ensure((size_t)m * 4 * 2));
            launch_byid_live(idx->del_dev.p, r0, m, map_of(F), map_of(F) + m, P.stream);
            d_rows = map_of(F);
        }
        launch_byid_gather(idx->corpus.p, idx->dtype, idx->ld, idx->dim, idx->count, idx->id_offset, nullptr, nullptr, d_rows, r0, F.live,
                           P.q_raw.as<float>(), nullptr, P.stream);   // (the range and the tombstones were checked on the host)
        HIP_TRY(hipGetLastError());
        return byid_search_begin(idx, P.q_raw.as<float>(), F.live, k1, idx->list_ids[c].as<uint64_t>(), idx->list_scores[c].as<float>());
    };
    auto finish = [&](const Flight& F) -> int {
        const uint32_t m = F.b.rows, c = F.b.slot;
        if (F.live) {
            VROD_TRY(search_end(idx));
            const vrod_search_stats& d = idx->stats;
            fold_stats(tot, d);
            tot.nq += d.nq;
            tot.scan_bytes += d.scan_bytes;
            tot.scan_flops += d.scan_flops;
            tot.overlap_ms += d.overlap_ms;
        }
        VROD_TRY(idx->byid_out_ids[c].ensure((size_t)m * k * 8));
        VROD_TRY(idx->byid_out_scores[c].ensure((size_t)m * k * 4));
        uint64_t* d_oi = idx->byid_out_ids[c].as<uint64_t>();
        float* d_os = idx->byid_out_scores[c].as<float>();
        // on the stream of the search just completed (the other slot's is scanning the next batch); a batch without a
        // search has no slot: the handle's own stream
        if (F.live)
            launch_byid_drop_self(idx->list_ids[c].as<uint64_t>(), idx->list_scores[c].as<float>(), k1, F.holes ? map_of(F) + m : nullptr, nullptr,
                                  idx->id_offset + row0 + F.b.first, m, k, d_oi, d_os, F.stream);
        else
            launch_fill_none(d_oi, d_os, (uint64_t)m * k, F.stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_ids + F.b.first * k, d_oi, (size_t)m * k * 8, hipMemcpyDeviceToHost, F.stream));
        HIP_TRY(hipMemcpyAsync(out_scores + F.b.first * k, d_os, (size_t)m * k * 4, hipMemcpyDeviceToHost, F.stream));
        HIP_TRY(hipStreamSynchronize(F.stream));
        return VROD_OK;
    };
    Flight cur{}, nxt{};
    int rc = begin(0, cur);
    for (uint64_t s = 0; rc == VROD_OK && s < nb; ++s) {
        const bool more = s + 1 < nb;
        if (more) rc = begin(s + 1, nxt);
        if (rc == VROD_OK) rc = finish(cur);
        cur = nxt;
    }
    if (rc != VROD_OK) {   // leave the handle idle: whatever is still pending is ended, the first error is the call's
        const std::string why = g_last_error;
        while (idx->n_pending()) (void)search_end(idx);
        g_last_error = why;
        return rc;
    }
    idx->stats = tot;
    return VROD_OK;
}

// ------------------------------------------------------------------ snapshots (vrod_index_save, vrod_index_load)
// The file format, its validation and the chunk arithmetic are snapshot_plan.h's, the kernels kernels_snapshot.hip's.
// Here: the file I/O and the two-buffer pipeline between the device and the file.
//   save   chunk c: pack kernel (rows -> dense staging, checksum) and the copy to pinned buffer c & 1 are enqueued on the
//          handle's stream; the host then writes chunk c - 1 from the other buffer while they run.
//   load   chunk c is read from the file into pinned buffer c & 1 while the copy to the device and the unpack kernel
//          (dense staging -> rows, checksum) of chunk c - 1 run.
// The side arrays take the same pipeline with a plain copy in place of the kernel and one checksum launch over the
// device array.  The checksums are taken on the device, over device memory, on both sides: HBM -> file -> HBM is covered
// end to end and the host makes no pass over the rows.  The bitmaps are the host mirrors' (the truth for both), checked
// on the host: a 32nd of a byte per row.
constexpr uint32_t kSnapSumWord = 32;   // idx->flags.p[32 .. 48): one 64-bit device sum per section kind (SNAP_KIND_END = 9)

static int snap_status(SnapStatus st, const char* path, const char* why) {
    if (st == SNAP_OK) return VROD_OK;
    return fail(st == SNAP_UNSUPPORTED ? VROD_ERR_UNSUPPORTED : VROD_ERR_CORRUPT, "%s: %s", path, why);
}

struct SnapFd {
    int fd = -1;
    ~SnapFd() { if (fd >= 0) (void)close(fd); }
};

static int snap_pwrite(int fd, const void* p, uint64_t n, uint64_t off) {
    const char* b = (const char*)p;
    while (n) {
        const ssize_t w = pwrite(fd, b, (size_t)n, (off_t)off);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return fail(VROD_ERR_IO, "writing the snapshot: %s", strerror(w < 0 ? errno : EIO));
        b += w; off += (uint64_t)w; n -= (uint64_t)w;
    }
    return VROD_OK;
}

// (the file's length was checked against its header: a short read means it shrank since)
static int snap_pread(int fd, void* p, uint64_t n, uint64_t off) {
    char* b = (char*)p;
    while (n) {
        const ssize_t r = pread(fd, b, (size_t)n, (off_t)off);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) return fail(VROD_ERR_IO, "reading the snapshot: %s", strerror(errno));
        if (r == 0) return fail(VROD_ERR_CORRUPT, "the snapshot ends before its header says (truncated)");
        b += r; off += (uint64_t)r; n -= (uint64_t)r;
    }
    return VROD_OK;
}

// Opens `path`, reads and validates its header block against the file's real length.  No device call.
static int snap_open(const char* path, SnapFd& f, SnapHeader& h) {
    f.fd = open(path, O_RDONLY | O_CLOEXEC);
    if (f.fd < 0) return fail(VROD_ERR_IO, "open %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(f.fd, &st) != 0) return fail(VROD_ERR_IO, "stat %s: %s", path, strerror(errno));
    if (!S_ISREG(st.st_mode)) return fail(VROD_ERR_IO, "%s is not a regular file", path);
    unsigned char block[kSnapBlock];
    uint64_t have = 0;
    while (have < kSnapBlock) {
        const ssize_t r = pread(f.fd, block + have, kSnapBlock - have, (off_t)have);
        if (r < 0 && errno == EINTR) continue;
        if (r < 0) return fail(VROD_ERR_IO, "read %s: %s", path, strerror(errno));
        if (r == 0) break;
        have += (uint64_t)r;
    }
    const char* why = "";
    return snap_status(snap_parse_header(block, have, (uint64_t)st.st_size, h, &why), path, why);
}

// The checksum of every section of at most max_bytes, on the host, 4 MiB at a time.
static int snap_verify_sections(int fd, const char* path, const SnapHeader& h, uint64_t max_bytes) {
    std::vector<unsigned char> buf;
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        const SnapSection& sec = h.sections[i];
        if (sec.bytes > max_bytes) continue;
        const uint64_t piece = 4ull << 20;
        buf.resize((size_t)std::min(piece, sec.bytes));
        uint64_t sum = 0;
        for (uint64_t off = 0; off < sec.bytes; off += piece) {
            const uint64_t n = std::min(piece, sec.bytes - off);
            VROD_TRY(snap_pread(fd, buf.data(), n, sec.offset + off));
            sum += snap_checksum(buf.data(), n, off / 4);
        }
        if (sum != sec.checksum) return fail(VROD_ERR_CORRUPT, "%s: checksum mismatch in section %u", path, sec.kind);
    }
    return VROD_OK;
}

// The deleted-row bits (a 32nd of a byte per row) name count - live_count rows.
static int snap_check_live(int fd, const char* path, const SnapHeader& h) {
    std::vector<uint32_t> del((size_t)((h.count + 31) / 32));
    VROD_TRY(snap_pread(fd, del.data(), del.size() * 4, h.find(SNAP_DELETED)->offset));
    if (h.count - snap_count_bits(del.data(), h.count) != h.live_count)
        return fail(VROD_ERR_CORRUPT, "%s: the deleted-row bits disagree with the live count", path);
    return VROD_OK;
}

// Two pinned host buffers and the events behind the device work that reads or writes each.  VROD_DEBUG_SNAPSHOT_TIMING=1:
// where a call's time went, one line on stderr -- the kernels and the copies by HIP events, the file I/O and the waits
// for the device by the host's clock.
struct SnapPipe {
    hipStream_t stream = nullptr;
    void* host[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t tm[2][3] = {};   // timing: [buffer][before the first step | between the two | behind the second]
    bool timing = false, used[2] = {false, false}, timed[2] = {false, false};
    size_t bytes = 0;
    double first_ms = 0, second_ms = 0, file_ms = 0, wait_ms = 0;
    std::chrono::steady_clock::time_point t_open;
    static double since(std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    }
    int open(hipStream_t s, size_t n) {
        stream = s;
        bytes = n;
        const char* e = getenv("VROD_DEBUG_SNAPSHOT_TIMING");
        timing = e && e[0] == '1';
        t_open = std::chrono::steady_clock::now();
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipHostMalloc(&host[b], n, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&ev[b], hipEventDisableTiming));
            if (timing) for (hipEvent_t& t : tm[b]) HIP_TRY(hipEventCreate(&t));
        }
        return VROD_OK;
    }
    int mark(int b, int i) {
        if (timing) { HIP_TRY(hipEventRecord(tm[b][i], stream)); if (i == 2) timed[b] = true; }
        return VROD_OK;
    }
    // the device is done with buffer b
    int wait(int b) {
        if (!used[b]) return VROD_OK;
        const auto t = std::chrono::steady_clock::now();
        HIP_TRY(hipEventSynchronize(ev[b]));
        wait_ms += since(t);
        used[b] = false;
        if (timed[b]) {
            float a = 0, c = 0;
            HIP_TRY(hipEventElapsedTime(&a, tm[b][0], tm[b][1]));
            HIP_TRY(hipEventElapsedTime(&c, tm[b][1], tm[b][2]));
            first_ms += a; second_ms += c;
            timed[b] = false;
        }
        return VROD_OK;
    }
    int submitted(int b) {
        HIP_TRY(hipEventRecord(ev[b], stream));
        used[b] = true;
        return VROD_OK;
    }
    void report(const char* what, const char* first, const char* second, uint64_t file_bytes) const {
        if (timing)
            fprintf(stderr, "{\"vrod_snapshot\": \"%s\", \"file_bytes\": %llu, \"total_ms\": %.3f, \"%s_ms\": %.3f, \"%s_ms\": %.3f, "
                    "\"file_ms\": %.3f, \"device_wait_ms\": %.3f}\n", what, (unsigned long long)file_bytes, since(t_open), first, first_ms,
                    second, second_ms, file_ms, wait_ms);
    }
    ~SnapPipe() {
        if (stream) (void)hipStreamSynchronize(stream);   // (a copy may still be aimed at a buffer)
        for (int b = 0; b < 2; ++b) {
            if (host[b]) (void)hipHostFree(host[b]);
            if (ev[b]) (void)hipEventDestroy(ev[b]);
            for (hipEvent_t t : tm[b]) if (t) (void)hipEventDestroy(t);
        }
    }
};

// `total` bytes in pieces of `piece` leave for the file at file_off: produce(off, n, b) enqueues whatever ends with bytes
// [off, off + n) in pinned buffer b; piece c + 1 is enqueued before the host waits for piece c and writes it.
template <typename F>
static int snap_stream_out(SnapPipe& P, int fd, uint64_t file_off, uint64_t total, uint64_t piece, F&& produce) {
    if (!total) return VROD_OK;
    const uint64_t n_pieces = (total + piece - 1) / piece;
    auto enqueue = [&](uint64_t c) -> int {
        const int b = (int)(c & 1);
        VROD_TRY(produce(c * piece, std::min(piece, total - c * piece), b));
        return P.submitted(b);
    };
    VROD_TRY(enqueue(0));
    for (uint64_t c = 0; c < n_pieces; ++c) {
        if (c + 1 < n_pieces) VROD_TRY(enqueue(c + 1));
        VROD_TRY(P.wait((int)(c & 1)));
        const auto t = std::chrono::steady_clock::now();
        VROD_TRY(snap_pwrite(fd, P.host[c & 1], std::min(piece, total - c * piece), file_off + c * piece));
        P.file_ms += SnapPipe::since(t);
    }
    return VROD_OK;
}

// The inverse: piece c is read into pinned buffer c & 1 (once the device is done with what it held), then consume(off, n,
// b) enqueues its way to the device; the read of piece c + 1 runs beside it.
template <typename F>
static int snap_stream_in(SnapPipe& P, int fd, uint64_t file_off, uint64_t total, uint64_t piece, F&& consume) {
    for (uint64_t c = 0; c * piece < total; ++c) {
        const int b = (int)(c & 1);
        const uint64_t n = std::min(piece, total - c * piece);
        VROD_TRY(P.wait(b));
        const auto t = std::chrono::steady_clock::now();
        VROD_TRY(snap_pread(fd, P.host[b], n, file_off + c * piece));
        P.file_ms += SnapPipe::since(t);
        VROD_TRY(consume(c * piece, n, b));
        VROD_TRY(P.submitted(b));
    }
    return VROD_OK;
}

// rows per chunk of a save or load of `count` rows (a small handle gets small buffers)
static uint64_t snap_chunk_rows_now(const vrod_index* idx, uint64_t count) {
    const char* e = getenv("VROD_DEBUG_SNAPSHOT_CHUNK_ROWS");   // read at every call: tests reach the chunk seams at small sizes
    return std::min(snap_chunk_rows(idx->dim, (uint32_t)idx->dtype, e ? strtoull(e, nullptr, 10) : 0), round_up(std::max<uint64_t>(count, 1), 32));
}
// bytes of one dense chunk in the staging buffers (whole words, whole 16-byte units)
static size_t snap_stage_bytes(const vrod_index* idx, uint64_t chunk_rows) { return (size_t)round_up(chunk_rows * idx->dim * idx->esize, 16); }

// the first ceil(count / 32) words of a host bitmap, the bits at and above `count` cleared
static std::vector<uint32_t> snap_bitmap(const std::vector<uint32_t>& bits, uint64_t count) {
    std::vector<uint32_t> w(bits.begin(), bits.begin() + (count + 31) / 32);
    if (count % 32) w.back() &= (1u << (count % 32)) - 1u;
    return w;
}

static int snap_save_body(vrod_index* idx, int fd) {
    VROD_TRY(set_device(idx));
    hipStream_t s = idx->stream;
    const uint64_t count = idx->count, es = idx->esize;
    SnapHeader h;
    h.dim = idx->dim; h.dtype = (uint32_t)idx->dtype; h.metric = (uint32_t)idx->metric;
    h.count = count; h.live_count = idx->live(); h.id_offset = idx->id_offset;
    auto add = [&](uint32_t kind) { h.sections[h.n_sections].kind = kind; h.sections[h.n_sections++].bytes = snap_section_bytes(kind, count, h.dim, h.dtype); };
    add(SNAP_ROWS); add(SNAP_NORMS); add(SNAP_DELETED);
    if (idx->filter_on) add(SNAP_FILTER);
    for_each_column(idx, [&](auto& c, int) { if (c.exists()) add(c.snap_kind); });
    snap_layout(h);
    if (ftruncate(fd, (off_t)h.file_bytes) != 0) return fail(VROD_ERR_IO, "sizing the snapshot: %s", strerror(errno));   // (the padding: zeros)

    const uint64_t chunk = snap_chunk_rows_now(idx, count);
    const size_t stage = snap_stage_bytes(idx, chunk);
    uint64_t* d_sum = (uint64_t*)(idx->flags.p + kSnapSumWord);
    uint64_t h_sum[SNAP_KIND_END] = {};
    {
        SnapPipe P;
        VROD_TRY(P.open(s, stage));
        VROD_TRY(idx->snap_stage.ensure(2 * stage));
        HIP_TRY(hipMemsetAsync(d_sum, 0, sizeof h_sum, s));
        HIP_TRY(hipMemcpyAsync(&h.max_xn2_bits, idx->max_xn2_bits, 4, hipMemcpyDeviceToHost, s));
        for (uint32_t i = 0; i < h.n_sections; ++i) {
            const SnapSection& sec = h.sections[i];
            if (sec.kind == SNAP_ROWS) {
                VROD_TRY(snap_stream_out(P, fd, sec.offset, sec.bytes, chunk * idx->dim * es, [&](uint64_t off, uint64_t n, int b) -> int {
                    const uint64_t r0 = off / (idx->dim * es), m = n / (idx->dim * es);
                    char* dense = idx->snap_stage.as<char>() + (size_t)b * stage;
                    VROD_TRY(P.mark(b, 0));
                    launch_snapshot_pack((const char*)idx->corpus.p + r0 * idx->row_bytes(), m, idx->dim, idx->ld, idx->dtype, dense, off / 4,
                                         d_sum + SNAP_ROWS, s);
                    HIP_TRY(hipGetLastError());
                    VROD_TRY(P.mark(b, 1));
                    HIP_TRY(hipMemcpyAsync(P.host[b], dense, round_up(n, 4), hipMemcpyDeviceToHost, s));
                    return P.mark(b, 2);
                }));
                continue;
            }
            const void* d_arr = sec.kind == SNAP_NORMS ? idx->xnorm2.p : nullptr;
            for_each_column(idx, [&](auto& c, int) { if (c.snap_kind == sec.kind) d_arr = c.dev.p; });
            if (!d_arr) continue;   // the bitmaps: below
            launch_snapshot_checksum(d_arr, sec.bytes, 0, d_sum + sec.kind, s);
            HIP_TRY(hipGetLastError());
            VROD_TRY(snap_stream_out(P, fd, sec.offset, sec.bytes, stage, [&](uint64_t off, uint64_t n, int b) -> int {
                HIP_TRY(hipMemcpyAsync(P.host[b], (const char*)d_arr + off, n, hipMemcpyDeviceToHost, s));
                return VROD_OK;
            }));
        }
        HIP_TRY(hipMemcpyAsync(h_sum, d_sum, sizeof h_sum, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        P.report("save", "pack_kernel", "copy_d2h", h.file_bytes);
    }
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        SnapSection& sec = h.sections[i];
        if (sec.kind == SNAP_DELETED || sec.kind == SNAP_FILTER) {
            const std::vector<uint32_t> w = snap_bitmap(sec.kind == SNAP_DELETED ? idx->del_bits : idx->allow_bits, count);
            sec.checksum = snap_checksum(w.data(), sec.bytes, 0);
            VROD_TRY(snap_pwrite(fd, w.data(), sec.bytes, sec.offset));
        } else {
            sec.checksum = h_sum[sec.kind];
        }
    }
    unsigned char block[kSnapBlock];
    snap_encode_header(h, block);
    VROD_TRY(snap_pwrite(fd, block, kSnapBlock, 0));
    if (fsync(fd) != 0) return fail(VROD_ERR_IO, "fsync of the snapshot: %s", strerror(errno));
    return VROD_OK;
}

// a column of a loaded handle: device copy and host mirror over the capacity, rows [0, count) from its section of the
// file, the rest at the column's default
template <typename T>
static int snap_load_column(vrod_index* idx, SnapPipe& P, int fd, const SnapSection& sec, RowColumn<T>& col, uint64_t* d_sum) {
    hipStream_t s = idx->stream;
    HIP_TRY(col.dev.alloc(idx->capacity * sizeof(T)));
    HIP_TRY(hipMemsetAsync(col.dev.p, col.fill_byte(), idx->capacity * sizeof(T), s));
    col.host.assign(idx->capacity, col.none);
    VROD_TRY(snap_stream_in(P, fd, sec.offset, sec.bytes, P.bytes / 8 * 8, [&](uint64_t off, uint64_t n, int b) -> int {
        memcpy((char*)col.host.data() + off, P.host[b], n);
        HIP_TRY(hipMemcpyAsync(col.dev.template get<char>() + off, P.host[b], n, hipMemcpyHostToDevice, s));
        return VROD_OK;
    }));
    launch_snapshot_checksum(col.dev.p, sec.bytes, 0, d_sum + sec.kind, s);
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}

// Fills a freshly created handle from an open, validated snapshot.
static int snap_load_body(vrod_index* idx, int fd, const char* path, const SnapHeader& h) {
    VROD_TRY(set_device(idx));
    hipStream_t s = idx->stream;
    const uint64_t count = h.count, es = idx->esize;
    idx->id_offset = h.id_offset;
    VROD_TRY(index_reserve(idx, count));   // every byte of the new allocations is zero: row padding, rows past the count

    // the bitmaps first, on the host
    const SnapSection* sec_del = h.find(SNAP_DELETED);
    VROD_TRY(snap_pread(fd, idx->del_bits.data(), sec_del->bytes, sec_del->offset));
    if (snap_checksum(idx->del_bits.data(), sec_del->bytes, 0) != sec_del->checksum)
        return fail(VROD_ERR_CORRUPT, "%s: checksum mismatch in section %u", path, (unsigned)SNAP_DELETED);
    if (count % 32) idx->del_bits[count / 32] &= (1u << (count % 32)) - 1u;
    const uint64_t n_deleted = snap_count_bits(idx->del_bits.data(), count);   // (checked against the live count before the device was opened)
    std::vector<uint32_t> allow;
    if (const SnapSection* sec = h.find(SNAP_FILTER)) {
        allow.resize((size_t)(sec->bytes / 4));
        VROD_TRY(snap_pread(fd, allow.data(), sec->bytes, sec->offset));
        if (snap_checksum(allow.data(), sec->bytes, 0) != sec->checksum)
            return fail(VROD_ERR_CORRUPT, "%s: checksum mismatch in section %u", path, (unsigned)SNAP_FILTER);
    }

    const uint64_t chunk = snap_chunk_rows_now(idx, count);
    const size_t stage = snap_stage_bytes(idx, chunk);
    uint64_t* d_sum = (uint64_t*)(idx->flags.p + kSnapSumWord);
    uint64_t h_sum[SNAP_KIND_END] = {};
    {
        SnapPipe P;
        VROD_TRY(P.open(s, stage));
        VROD_TRY(idx->snap_stage.ensure(2 * stage));
        HIP_TRY(hipMemsetAsync(d_sum, 0, sizeof h_sum, s));
        const SnapSection* rows = h.find(SNAP_ROWS);
        VROD_TRY(snap_stream_in(P, fd, rows->offset, rows->bytes, chunk * idx->dim * es, [&](uint64_t off, uint64_t n, int b) -> int {
            const uint64_t r0 = off / (idx->dim * es), m = n / (idx->dim * es);
            char* dense = idx->snap_stage.as<char>() + (size_t)b * stage;
            if (n % 4) memset((char*)P.host[b] + n, 0, 4 - n % 4);   // the zero fill of the payload's last word
            VROD_TRY(P.mark(b, 0));
            HIP_TRY(hipMemcpyAsync(dense, P.host[b], round_up(n, 4), hipMemcpyHostToDevice, s));
            VROD_TRY(P.mark(b, 1));
            launch_snapshot_unpack(dense, m, idx->dim, idx->ld, idx->dtype, (char*)idx->corpus.p + r0 * idx->row_bytes(), off / 4,
                                   d_sum + SNAP_ROWS, s);
            HIP_TRY(hipGetLastError());
            return P.mark(b, 2);
        }));
        const SnapSection* norms = h.find(SNAP_NORMS);
        VROD_TRY(snap_stream_in(P, fd, norms->offset, norms->bytes, stage / 4 * 4, [&](uint64_t off, uint64_t n, int b) -> int {
            HIP_TRY(hipMemcpyAsync((char*)idx->xnorm2.p + off, P.host[b], n, hipMemcpyHostToDevice, s));
            return VROD_OK;
        }));
        launch_snapshot_checksum(idx->xnorm2.p, norms->bytes, 0, d_sum + SNAP_NORMS, s);
        HIP_TRY(hipGetLastError());
        int col_rc = VROD_OK;
        for_each_column(idx, [&](auto& c, int) {
            const SnapSection* sec = h.find(c.snap_kind);
            if (sec && col_rc == VROD_OK) col_rc = snap_load_column(idx, P, fd, *sec, c, d_sum);
        });
        VROD_TRY(col_rc);
        HIP_TRY(hipMemcpyAsync(idx->max_xn2_bits, &h.max_xn2_bits, 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(h_sum, d_sum, sizeof h_sum, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        P.report("load", "copy_h2d", "unpack_kernel", h.file_bytes);
    }
    for (uint32_t i = 0; i < h.n_sections; ++i) {
        const SnapSection& sec = h.sections[i];
        if (sec.kind == SNAP_DELETED || sec.kind == SNAP_FILTER) continue;
        if (h_sum[sec.kind] != sec.checksum)
            return fail(VROD_ERR_CORRUPT, "%s: checksum mismatch in section %u (as it arrived in device memory)", path, sec.kind);
    }
    idx->count = count;
    if (n_deleted) {
        HIP_TRY(idx->del_dev.alloc(idx->del_bits.size() * 4));
        HIP_TRY(hipMemcpy(idx->del_dev.p, idx->del_bits.data(), idx->del_bits.size() * 4, hipMemcpyHostToDevice));
        idx->n_deleted = n_deleted;
        mask_changed(idx);
    }
    // rows the filter does not name are not allowed, so the file's ceil(count / 32) words over `count` rows give the
    // effective mask and the eligible count the saved handle had, whatever n_rows its filter was set with
    if (h.find(SNAP_FILTER)) {
        static const uint32_t kNone = 0u;
        VROD_TRY(index_set_filter(idx, count ? allow.data() : &kNone, count));
    }
    // the key table is not in the file: it is built from the key column and the deleted-row bits, which is also the
    // check that no two live rows of the file share a key
    if (idx->keys.exists()) {
        for (uint64_t r = 0; r < count; ++r) idx->keyed_live += idx->keys.host[r] != kKeyNone && !bit_of(idx->del_bits.data(), r);
        bool dup = false;
        VROD_TRY(keys_rebuild(idx, idx->keyed_live, false, "vrod_index_load", &dup));
        if (dup) return fail(VROD_ERR_CORRUPT, "%s: two live rows hold the same key", path);
    }
    return VROD_OK;
}

// ------------------------------------------------------------------ C ABI
extern "C" {

const char* vrod_last_error(void) { return g_last_error.c_str(); }
#ifndef VROD_HIPCC_VERSION
#define VROD_HIPCC_VERSION "unknown"
#endif
// names the compiler that built the device code: the 4-wave scan's register audit was run on THAT compiler's output
const char* vrod_version(void) { return "vrod_amd 0.3 (gfx950; hipcc " VROD_HIPCC_VERSION "; w4 accumulator audit passed at build)"; }

int vrod_index_create(vrod_index** out, uint32_t dim, int dtype, int metric, const int* device_ids,
                      int n_devices) {
    if (!out) return fail(VROD_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (dim == 0 || dim > VROD_MAX_DIM) return fail(VROD_ERR_INVALID_ARG, "dim must be in 1..%u", VROD_MAX_DIM);
    if (dtype != VROD_DTYPE_F32 && dtype != VROD_DTYPE_BF16) return fail(VROD_ERR_INVALID_ARG, "bad dtype %d", dtype);
    if (!valid_metric(metric)) return fail(VROD_ERR_INVALID_ARG, "bad metric %d", metric);
    if (n_devices < 0 || (n_devices > 0 && !device_ids)) return fail(VROD_ERR_INVALID_ARG, "bad device list");
    if (n_devices > 1) {
        if (n_devices > 64) return fail(VROD_ERR_INVALID_ARG, "at most 64 devices per handle");
        vrod_index* c = new (std::nothrow) vrod_index();
        if (!c) return fail(VROD_ERR_OUT_OF_MEMORY, "host allocation failed");
        c->dim = dim; c->dtype = dtype; c->metric = metric;
        for (int g = 0; g < n_devices; ++g) {
            vrod_index* sh = nullptr;
            const int rc = vrod_index_create(&sh, dim, dtype, metric, &device_ids[g], 1);
            if (rc != VROD_OK) { vrod_index_destroy(c); return rc; }
            c->shards.push_back(sh);
        }
        c->device = c->shards[0]->device;
        c->ld = c->shards[0]->ld; c->esize = c->shards[0]->esize;
        const int rc = composite_open_exchange(c);
        if (rc != VROD_OK) { const std::string why = g_last_error; vrod_index_destroy(c); g_last_error = why; return rc; }
        *out = c;
        return VROD_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(VROD_ERR_NO_DEVICE, "no HIP device visible: libvrod_hip has no CPU fallback");
    const int dev = n_devices == 1 ? device_ids[0] : 0;
    if (dev < 0 || dev >= ndev) return fail(VROD_ERR_INVALID_ARG, "device %d out of range (have %d)", dev, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(VROD_ERR_NO_DEVICE, "device %d is %s; libvrod_hip is built for gfx950 (MI355X) only", dev, prop.gcnArchName);
    vrod_index* idx = new (std::nothrow) vrod_index();
    if (!idx) return fail(VROD_ERR_OUT_OF_MEMORY, "host allocation failed");
    idx->device = dev;
    idx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    idx->dim = dim;
    idx->dtype = dtype;
    idx->metric = metric;
    idx->esize = dtype == VROD_DTYPE_BF16 ? 2 : 4;
    // rows are padded to whole 128-B lines: 64 bf16 / 32 fp32 elements
    idx->ld = (uint32_t)round_up(dim, dtype == VROD_DTYPE_BF16 ? 64 : 32);
    idx->ldp = (uint32_t)round_up(dim, 64);
    {
        const char* e = getenv("VROD_F32_SPLIT");
        idx->split_enabled = dtype == VROD_DTYPE_F32 && !(e && e[0] == '0');
        idx->split_forced = idx->split_enabled && e && e[0] == '1';
    }
    int rc = VROD_OK;
    do {
        if (hipSetDevice(dev) != hipSuccess) { rc = fail(VROD_ERR_HIP, "hipSetDevice failed"); break; }
        if (hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(VROD_ERR_HIP, "hipStreamCreate failed"); break; }
        if (idx->flags.alloc(8192) != hipSuccess) { rc = fail(VROD_ERR_OUT_OF_MEMORY, "hipMalloc failed"); break; }
        if (hipMemset(idx->flags.p, 0, 8192) != hipSuccess) { rc = fail(VROD_ERR_HIP, "hipMemset failed"); break; }
        idx->max_xn2_bits = idx->flags.p + 8;
        for (Pending& P : idx->slot) {
            if (hipStreamCreateWithFlags(&P.stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(VROD_ERR_HIP, "hipStreamCreate failed"); break; }
            if (P.flags.alloc(kSlotFlagBytes) != hipSuccess) { rc = fail(VROD_ERR_OUT_OF_MEMORY, "hipMalloc failed"); break; }
            if (hipMemset(P.flags.p, 0, kSlotFlagBytes) != hipSuccess) { rc = fail(VROD_ERR_HIP, "hipMemset failed"); break; }
            if (hipEventCreateWithFlags(&P.done, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&P.scans_done, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&P.mid_done, hipEventDisableTiming) != hipSuccess) { rc = fail(VROD_ERR_HIP, "hipEventCreate failed"); break; }
        }
    } while (0);
    if (rc != VROD_OK) { vrod_index_destroy(idx); return rc; }
    *out = idx;
    return VROD_OK;
}

// Orders the teardown; the handle's buffers free themselves when it is deleted, under the device set just before.
int vrod_index_destroy(vrod_index* idx) {
    if (!idx) return VROD_OK;
    if (idx->composite()) {
        while (idx->n_pending()) (void)composite_end(idx, nullptr, nullptr);   // a begun search is ended before its buffers go
        for (size_t g = 0; g < idx->shards.size(); ++g) {   // (buffers on the shards' devices: released under them)
            (void)hipSetDevice(idx->shards[g]->device);
            for (int c = 0; c < 2; ++c)
                if (g < idx->sh_q[c].size()) idx->sh_q[c][g].release();
        }
        for (auto& D : idx->groups) {
            (void)hipSetDevice(D.device);
            if (D.xstream) (void)hipStreamSynchronize(D.xstream);
            if (D.comm) (void)rccl_api().CommDestroy(D.comm);
            for (int c = 0; c < 2; ++c) { D.send[c].release(); D.recv[c].release(); }
            if (D.xstream) (void)hipStreamDestroy(D.xstream);
        }
        for (vrod_index* sh : idx->shards) vrod_index_destroy(sh);
        (void)hipSetDevice(idx->device);
        if (idx->caller_ev) (void)hipEventDestroy(idx->caller_ev);
        for (auto& CP : idx->cslot) if (CP.caller_ev) (void)hipEventDestroy(CP.caller_ev);
        delete idx;
        return VROD_OK;
    }
    (void)hipSetDevice(idx->device);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    for (Pending& P : idx->slot)
        if (P.stream) (void)hipStreamSynchronize(P.stream);
    for (Pending& P : idx->slot) {
        if (P.stream) (void)hipStreamDestroy(P.stream);
        if (P.gexec) (void)hipGraphExecDestroy(P.gexec);
        for (hipEvent_t e : P.ev) (void)hipEventDestroy(e);
        if (P.done) (void)hipEventDestroy(P.done);
        if (P.scans_done) (void)hipEventDestroy(P.scans_done);
        if (P.mid_done) (void)hipEventDestroy(P.mid_done);
        if (P.h_readback) (void)hipHostFree(P.h_readback);
    }
    for (auto& T : idx->tail_ev) { if (T.start) (void)hipEventDestroy(T.start); if (T.stop) (void)hipEventDestroy(T.stop); }
    if (idx->caller_ev) (void)hipEventDestroy(idx->caller_ev);
    if (idx->stream) (void)hipStreamDestroy(idx->stream);
    delete idx;
    return VROD_OK;
}

int vrod_index_reserve(vrod_index* idx, uint64_t n_rows) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    if (idx->composite()) {
        const uint64_t G = idx->shards.size();
        const uint64_t per = (n_rows / (kShardBlock * G) + 1) * kShardBlock;   // whole blocks per shard
        for (vrod_index* sh : idx->shards) VROD_TRY(vrod_index_reserve(sh, per));
        return VROD_OK;
    }
    VROD_TRY(require_idle(idx, "vrod_index_reserve"));
    VROD_TRY(set_device(idx));
    return index_reserve(idx, n_rows);
}

int vrod_index_add(vrod_index* idx, const float* rows, uint64_t n) {
    if (!idx || (!rows && n)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    const RowSource src = rows_on_host(rows, idx->dim);
    if (idx->composite()) return composite_add(idx, src, n);
    VROD_TRY(require_idle(idx, "vrod_index_add"));
    return index_add(idx, src, n);
}

int vrod_index_add_synthetic(vrod_index* idx, uint64_t seed, uint64_t first_row, uint64_t n) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    const RowSource src = rows_synthetic(seed, first_row);
    if (idx->composite()) return composite_add(idx, src, n);
    VROD_TRY(require_idle(idx, "vrod_index_add_synthetic"));
    return index_add(idx, src, n);
}

int vrod_index_count(const vrod_index* idx, uint64_t* out_count) {
    if (!idx || !out_count) return fail(VROD_ERR_INVALID_ARG, "null argument");
    *out_count = idx->count;
    return VROD_OK;
}

int vrod_index_delete(vrod_index* idx, const uint64_t* ids, uint64_t n) {
    if (!idx || (!ids && n)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    VROD_TRY(require_idle(idx, "vrod_index_delete"));
    for (uint64_t i = 0; i < n; ++i)   // the whole call or nothing
        if (ids[i] < idx->id_offset || ids[i] - idx->id_offset >= idx->count)
            return fail(VROD_ERR_INVALID_ARG, "id %llu is not a row of this handle (ids %llu..%llu)", (unsigned long long)ids[i],
                        (unsigned long long)idx->id_offset, (unsigned long long)(idx->id_offset + idx->count));
    if (!n) return VROD_OK;
    if (idx->composite()) return composite_delete(idx, ids, n);
    std::vector<uint64_t> rows(ids, ids + n);
    for (uint64_t& r : rows) r -= idx->id_offset;
    return index_delete_rows(idx, rows);
}

// vrod_index_update behind its argument checks; ids: host memory
static int update_checked(vrod_index* idx, const uint64_t* ids, const RowSource& src, uint64_t n) {
    const size_t G = idx->shards.size();
    std::vector<uint64_t> rows_of(n);
    for (uint64_t i = 0; i < n; ++i) {   // the whole call or nothing
        const uint64_t r = ids[i] - idx->id_offset;
        bool current = ids[i] >= idx->id_offset && r < idx->count;
        if (current) {
            const vrod_index* sh = G ? idx->shards[(size_t)((r / kShardBlock) % G)] : idx;
            current = !bit_of(sh->del_bits.data(), G ? local_row_of(idx, r) : r);
        }
        if (!current)
            return fail(VROD_ERR_INVALID_ARG, "id %llu is not a current row of this handle (ids %llu..%llu, deleted rows excluded)",
                        (unsigned long long)ids[i], (unsigned long long)idx->id_offset, (unsigned long long)(idx->id_offset + idx->count));
        rows_of[i] = r;
    }
    if (!n) return VROD_OK;
    // an id named twice: the last occurrence wins, the earlier ones are prepared and checked but written nowhere
    std::vector<bool> seen(idx->count, false), skip(n, false);
    for (uint64_t i = n; i-- > 0;) {
        if (seen[rows_of[i]]) skip[i] = true;
        seen[rows_of[i]] = true;
    }
    if (G) return composite_update(idx, rows_of, skip, src);
    std::vector<uint32_t> dst(n);
    for (uint64_t i = 0; i < n; ++i) dst[i] = skip[i] ? kScatterSkip : (uint32_t)rows_of[i];
    return index_update(idx, dst, src, n);
}

int vrod_index_update(vrod_index* idx, const uint64_t* ids, const float* rows, uint64_t n) {
    if (!idx || ((!ids || !rows) && n)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    VROD_TRY(require_idle(idx, "vrod_index_update"));
    return update_checked(idx, ids, rows_on_host(rows, idx->dim), n);
}

// ------------------------------------------------------------------ device-resident ingest: add / update / get_rows
// What the three _device forms that take rows check before any device call.
static int check_ingest_args(const vrod_index* idx, const char* what, const void* d_rows, int src_dtype, uint64_t row_stride, uint64_t n) {
    if (!ingest_dtype_known(src_dtype)) return fail(VROD_ERR_INVALID_ARG, "%s: unknown src_dtype %d", what, src_dtype);
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "%s: idx is null", what);
    if (!d_rows && n) return fail(VROD_ERR_INVALID_ARG, "%s: d_rows is null", what);
    switch (ingest_check_layout((uint64_t)(uintptr_t)d_rows, src_dtype, row_stride, idx->dim, n)) {
        case INGEST_OK: return VROD_OK;
        case INGEST_BAD_STRIDE:
            return fail(VROD_ERR_INVALID_ARG, "%s: row_stride %llu is less than dim %u", what, (unsigned long long)row_stride, idx->dim);
        case INGEST_OVERFLOW: return fail(VROD_ERR_INVALID_ARG, "%s: n * row_stride overflows 64 bits", what);
        default: return fail(VROD_ERR_INVALID_ARG, "%s: d_rows is not aligned to its element", what);
    }
}

// The stream rule of the synchronous device forms (begin_sync_device), then where the caller's rows live.
static int ingest_open(vrod_index* idx, const char* what, const void* d_ptr, void* stream, int* device) {
    VROD_TRY(set_device(idx));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, d_ptr) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(VROD_ERR_INVALID_ARG, "%s: the rows are not in device memory", what);
    }
    *device = at.device;
    return VROD_OK;
}

int vrod_index_add_device(vrod_index* idx, const void* d_rows, int src_dtype, uint64_t row_stride, uint64_t n, void* stream) {
    VROD_TRY(check_ingest_args(idx, "vrod_index_add_device", d_rows, src_dtype, row_stride, n));
    VROD_TRY(require_idle(idx, "vrod_index_add_device"));
    if (!n) return VROD_OK;
    RowSource src = rows_on_device(d_rows, src_dtype, row_stride);
    VROD_TRY(ingest_open(idx, "vrod_index_add_device", d_rows, stream, &src.device));
    if (idx->composite()) return composite_add(idx, src, n);
    return index_add(idx, src, n);
}

int vrod_index_update_device(vrod_index* idx, const uint64_t* d_ids, const void* d_rows, int src_dtype, uint64_t row_stride, uint64_t n,
                             void* stream) {
    VROD_TRY(check_ingest_args(idx, "vrod_index_update_device", d_rows, src_dtype, row_stride, n));
    if (!d_ids && n) return fail(VROD_ERR_INVALID_ARG, "vrod_index_update_device: d_ids is null");
    VROD_TRY(require_idle(idx, "vrod_index_update_device"));
    if (!n) return VROD_OK;
    RowSource src = rows_on_device(d_rows, src_dtype, row_stride);
    VROD_TRY(ingest_open(idx, "vrod_index_update_device", d_rows, stream, &src.device));
    std::vector<uint64_t> ids(n);   // 8 bytes per row cross to the host for the host form's checks; the rows stay
    HIP_TRY(hipMemcpy(ids.data(), d_ids, n * 8, hipMemcpyDeviceToHost));
    return update_checked(idx, ids.data(), src, n);
}

// Rows [first, first + m) of a single-device handle (or shard) as fp32 at d_out, out_stride floats apart.
static int get_rows_to_device(vrod_index* idx, uint64_t first, uint64_t m, float* d_out, uint64_t out_stride, int out_device) {
    VROD_TRY(set_device(idx));
    const char* rows = (const char*)idx->corpus.p + first * idx->row_bytes();
    if (out_device == idx->device && !ingest_force_stage()) {
        launch_rows_get_strided(rows, idx->dtype, m, idx->dim, idx->ld, d_out, out_stride, idx->stream);
        HIP_TRY(hipGetLastError());
    } else {   // the output lives on another device: dense rows here, then a pitched copy
        VROD_TRY(idx->raw_stage.ensure(m * idx->dim * 4));
        launch_rows_get_strided(rows, idx->dtype, m, idx->dim, idx->ld, idx->raw_stage.as<float>(), idx->dim, idx->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy2DAsync(d_out, out_stride * 4, idx->raw_stage.p, (size_t)idx->dim * 4, (size_t)idx->dim * 4, m, hipMemcpyDeviceToDevice,
                                 idx->stream));
    }
    HIP_TRY(hipStreamSynchronize(idx->stream));
    return VROD_OK;
}

int vrod_index_get_rows_device(vrod_index* idx, uint64_t first, uint64_t n, float* d_out_rows, uint64_t out_row_stride, void* stream) {
    VROD_TRY(check_ingest_args(idx, "vrod_index_get_rows_device", d_out_rows, SRC_F32, out_row_stride, n));
    if (first > idx->count || n > idx->count - first)
        return fail(VROD_ERR_INVALID_ARG, "rows [%llu, %llu) out of range", (unsigned long long)first, (unsigned long long)(first + n));
    VROD_TRY(require_idle(idx, "vrod_index_get_rows_device"));
    if (!n) return VROD_OK;
    int out_device = 0;
    VROD_TRY(ingest_open(idx, "vrod_index_get_rows_device", d_out_rows, stream, &out_device));
    if (!idx->composite()) return get_rows_to_device(idx, first, n, d_out_rows, out_row_stride, out_device);
    return for_each_piece(idx, first, n, [&](size_t g, uint64_t r, uint64_t m) {
        return get_rows_to_device(idx->shards[g], local_row_of(idx, r), m, d_out_rows + (r - first) * out_row_stride, out_row_stride, out_device);
    });
}

int vrod_index_compact(vrod_index* idx, uint64_t* out_new_ids, uint64_t map_len) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    VROD_TRY(require_idle(idx, "vrod_index_compact"));
    if (idx->composite())
        return fail(VROD_ERR_UNSUPPORTED, "vrod_index_compact on a multi-device handle: renumbering would re-deal the rows across the devices");
    if (out_new_ids && map_len != idx->count)
        return fail(VROD_ERR_INVALID_ARG, "an id map of %llu entries for a handle of %llu rows", (unsigned long long)map_len, (unsigned long long)idx->count);
    return index_compact(idx, out_new_ids);
}

int vrod_index_live_count(const vrod_index* idx, uint64_t* out) {
    if (!idx || !out) return fail(VROD_ERR_INVALID_ARG, "null argument");
    uint64_t dead = idx->n_deleted;
    for (const vrod_index* sh : idx->shards) dead += sh->n_deleted;
    *out = idx->count - dead;
    return VROD_OK;
}

int vrod_index_set_filter(vrod_index* idx, const uint32_t* allow_words, uint64_t n_rows) {
    if (!idx || (!allow_words && n_rows)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    VROD_TRY(require_idle(idx, "vrod_index_set_filter"));
    if (n_rows > idx->count)
        return fail(VROD_ERR_INVALID_ARG, "a filter of %llu rows on a handle of %llu", (unsigned long long)n_rows, (unsigned long long)idx->count);
    static const uint32_t kNone = 0u;   // (p, 0): a filter that allows nothing
    const uint32_t* allow = allow_words ? allow_words : nullptr;
    if (allow_words && !n_rows) allow = &kNone;
    if (idx->composite()) return composite_set_filter(idx, allow, n_rows);
    return index_set_filter(idx, allow, n_rows);
}

int vrod_index_filter_count(const vrod_index* idx, uint64_t* out) {
    if (!idx || !out) return fail(VROD_ERR_INVALID_ARG, "null argument");
    if (!idx->composite()) { *out = idx->eligible(); return VROD_OK; }
    uint64_t n = 0;
    for (const vrod_index* sh : idx->shards) n += sh->eligible();
    *out = n;
    return VROD_OK;
}

int vrod_index_set_id_offset(vrod_index* idx, uint64_t offset) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    idx->id_offset = offset;
    return VROD_OK;
}

int vrod_index_get_rows(vrod_index* idx, uint64_t first, uint64_t n, float* out_rows) {
    if (!idx || (!out_rows && n)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    if (first + n > idx->count) return fail(VROD_ERR_INVALID_ARG, "rows [%llu, %llu) out of range", (unsigned long long)first, (unsigned long long)(first + n));
    if (!n) return VROD_OK;
    if (idx->composite()) return composite_get_rows(idx, first, n, out_rows);
    VROD_TRY(require_idle(idx, "vrod_index_get_rows"));
    VROD_TRY(set_device(idx));
    VROD_TRY(idx->raw_stage.ensure(n * idx->dim * 4));
    launch_rows_get_strided((const char*)idx->corpus.p + first * idx->row_bytes(), idx->dtype, n, idx->dim, idx->ld, idx->raw_stage.as<float>(),
                            idx->dim, idx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_rows, idx->raw_stage.p, n * idx->dim * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    return VROD_OK;
}

// [first_id, first_id + n) are ids of this handle's rows (n = 0 at the end of them included)
static int check_id_range(const vrod_index* idx, uint64_t first_id, uint64_t n) {
    if (first_id < idx->id_offset || first_id - idx->id_offset > idx->count || n > idx->count - (first_id - idx->id_offset))
        return fail(VROD_ERR_INVALID_ARG, "ids [%llu, %llu) are not all rows of this handle (ids %llu..%llu)", (unsigned long long)first_id,
                    (unsigned long long)(first_id + n), (unsigned long long)idx->id_offset, (unsigned long long)(idx->id_offset + idx->count));
    return VROD_OK;
}

// The handle's own top-k result rows, which a host form's search writes: grown for nq * k, and copied out to the caller.
static int grow_topk_out(vrod_index* idx, uint32_t nq, uint32_t k) {
    VROD_TRY(idx->out_ids.ensure((size_t)nq * k * 8));
    VROD_TRY(idx->out_scores.ensure((size_t)nq * k * 4));
    return VROD_OK;
}
static int copy_topk_out(vrod_index* idx, uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores) {
    HIP_TRY(hipMemcpy(out_ids, idx->out_ids.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_scores, idx->out_scores.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    return VROD_OK;
}

// What every synchronous device form starts with: the handle idle, its device current, and -- as a range search --
// whatever the caller's stream holds complete before the library's streams start.
static int begin_sync_device(vrod_index* idx, const char* what, void* stream) {
    VROD_TRY(require_idle(idx, what));
    VROD_TRY(set_device(idx));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return VROD_OK;
}

static int check_search_args(vrod_index* idx, const void* q, uint32_t nq, uint32_t k, const void* oi, const void* os) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    if (nq && (!q || !oi || !os)) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    if (k == 0 || k > VROD_MAX_K) return fail(VROD_ERR_INVALID_ARG, "k must be in 1..%u", VROD_MAX_K);
    return VROD_OK;
}

// The arguments of a derived search, refused in this order: a null handle; a null pointer of `first` (all are needed once
// nq is not zero); k, where the call has one that is checked here; a null pointer of `then`; a composite handle, as
// "<what> on a multi-device handle: <why_not>".
static const char kLabelsNotRouted[] = "labels are not routed to the shards", kTagsNotRouted[] = "tags are not routed to the shards",
                  kRowsNotGathered[] = "stored rows are not gathered across the shards",
                  kCandidatesNotRouted[] = "candidate ids are not routed to the shards";
static int check_derived_args(vrod_index* idx, const char* what, const char* why_not, uint32_t nq, std::initializer_list<const void*> first,
                              bool has_k, uint32_t k, std::initializer_list<const void*> then = {}) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    for (const void* p : first)
        if (nq && !p) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    if (has_k && (k == 0 || k > VROD_MAX_K)) return fail(VROD_ERR_INVALID_ARG, "k must be in 1..%u", VROD_MAX_K);
    for (const void* p : then)
        if (nq && !p) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "%s on a multi-device handle: %s", what, why_not);
    return VROD_OK;
}

// What the host form of a derived search starts with: the handle idle, its device current, the caller's n raw vectors
// in host_q (vecs null: room for them, nothing copied) and the handle's top-k result rows grown (k = 0: the call has
// none); copy_topk_out ends it.  A form that validates host arrays behind the idle check makes that check itself first.
static int begin_host_form(vrod_index* idx, const char* what, const float* vecs, size_t n, uint32_t nq, uint32_t k) {
    VROD_TRY(require_idle(idx, what));
    VROD_TRY(set_device(idx));
    VROD_TRY(idx->host_q.ensure(n * idx->dim * 4));
    if (k) VROD_TRY(grow_topk_out(idx, nq, k));
    if (vecs && n) HIP_TRY(hipMemcpy(idx->host_q.p, vecs, n * idx->dim * 4, hipMemcpyHostToDevice));
    return VROD_OK;
}

// A device form's lims array [nq + 1], read to the host.
static int read_lims(const uint32_t* d_lims, uint32_t nq, std::vector<uint32_t>& lims) {
    lims.resize((size_t)nq + 1);
    HIP_TRY(hipMemcpy(lims.data(), d_lims, lims.size() * 4, hipMemcpyDeviceToHost));
    return VROD_OK;
}

// `id` names a live row of this handle (kind: what the message calls it).  The host mirror of the tombstones is the
// truth: a host form launches nothing for a bad id.
static int check_live_id(const vrod_index* idx, uint64_t id, const char* kind) {
    if (id < idx->id_offset || id - idx->id_offset >= idx->count || bit_of(idx->del_bits.data(), id - idx->id_offset))
        return fail(VROD_ERR_INVALID_ARG, "%s %llu is not a live row of this handle (ids %llu..%llu, deleted rows excluded)", kind,
                    (unsigned long long)id, (unsigned long long)idx->id_offset, (unsigned long long)(idx->id_offset + idx->count));
    return VROD_OK;
}

int vrod_search_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k,
                       uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    VROD_TRY(check_search_args(idx, d_queries, nq, k, d_out_ids, d_out_scores));
    if (idx->composite())   // pointers on the first device of the handle
        return composite_search(idx, d_queries, false, 0, 0, nq, k, d_out_ids, d_out_scores, stream);
    VROD_TRY(require_idle(idx, "vrod_search_device"));
    VROD_TRY(set_device(idx));
    VROD_TRY(order_after_caller(idx, stream));   // the caller's inputs are ready
    return run_search(idx, d_queries, nq, k, d_out_ids, d_out_scores);
}

int vrod_search_begin_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k,
                             uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    VROD_TRY(check_search_args(idx, d_queries, nq, k, d_out_ids, d_out_scores));
    if (idx->composite()) return composite_begin(idx, d_queries, false, 0, 0, nq, k, d_out_ids, d_out_scores, stream);
    VROD_TRY(set_device(idx));
    VROD_TRY(order_after_caller(idx, stream));
    return search_begin(idx, d_queries, nq, k, d_out_ids, d_out_scores);
}

int vrod_search_begin_synthetic_device(vrod_index* idx, uint64_t seed, uint64_t first_row, uint32_t nq,
                                       uint32_t k, uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    VROD_TRY(check_search_args(idx, (void*)1, nq, k, d_out_ids, d_out_scores));
    if (idx->composite()) return composite_begin(idx, nullptr, false, seed, first_row, nq, k, d_out_ids, d_out_scores, stream);
    if (idx->n_pending() >= 2) return fail(VROD_ERR_INVALID_ARG, "two searches are already pending: call vrod_search_end first");
    VROD_TRY(set_device(idx));
    VROD_TRY(order_after_caller(idx, stream));
    // the raw queries are consumed by the prepare launch of this same search: one shared buffer,
    // stream-ordered (a regrowth frees it through hipFree, which waits for the device)
    Pending& P = next_slot(idx);
    VROD_TRY(P.q_raw.ensure((size_t)std::max<uint32_t>(nq, 1) * idx->dim * 4));
    launch_synth_rows(seed, first_row, nq, idx->dim, P.q_raw.as<float>(), P.stream);
    return search_begin(idx, P.q_raw.as<float>(), nq, k, d_out_ids, d_out_scores);
}

int vrod_search_end(vrod_index* idx) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    if (idx->composite()) return composite_end(idx, nullptr, nullptr);
    VROD_TRY(set_device(idx));
    return search_end(idx);
}

int vrod_search_pending(const vrod_index* idx, uint32_t* out_pending) {
    if (!idx || !out_pending) return fail(VROD_ERR_INVALID_ARG, "null argument");
    *out_pending = idx->n_pending();
    return VROD_OK;
}

int vrod_search_synthetic_device(vrod_index* idx, uint64_t seed, uint64_t first_row, uint32_t nq,
                                 uint32_t k, uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    VROD_TRY(check_search_args(idx, (void*)1, nq, k, d_out_ids, d_out_scores));
    if (idx->composite())   // every device generates the batch's queries itself: nothing to copy
        return composite_search(idx, nullptr, false, seed, first_row, nq, k, d_out_ids, d_out_scores, stream);
    VROD_TRY(require_idle(idx, "vrod_search_synthetic_device"));
    VROD_TRY(set_device(idx));
    VROD_TRY(order_after_caller(idx, stream));
    Pending& P = next_slot(idx);
    VROD_TRY(P.q_raw.ensure((size_t)std::max<uint32_t>(nq, 1) * idx->dim * 4));
    launch_synth_rows(seed, first_row, nq, idx->dim, P.q_raw.as<float>(), P.stream);
    return run_search(idx, P.q_raw.as<float>(), nq, k, d_out_ids, d_out_scores);
}

int vrod_search(vrod_index* idx, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_ids,
                float* out_scores) {
    VROD_TRY(check_search_args(idx, queries, nq, k, out_ids, out_scores));
    if (!nq) return VROD_OK;
    if (idx->composite()) return composite_search(idx, queries, true, 0, 0, nq, k, out_ids, out_scores, nullptr);
    VROD_TRY(require_idle(idx, "vrod_search"));
    VROD_TRY(set_device(idx));
    Pending& P = next_slot(idx);
    VROD_TRY(P.q_raw.ensure((size_t)nq * idx->dim * 4));
    VROD_TRY(grow_topk_out(idx, nq, k));
    HIP_TRY(hipMemcpyAsync(P.q_raw.p, queries, (size_t)nq * idx->dim * 4, hipMemcpyHostToDevice, P.stream));
    VROD_TRY(run_search(idx, P.q_raw.as<float>(), nq, k, idx->out_ids.as<uint64_t>(), idx->out_scores.as<float>()));
    HIP_TRY(hipMemcpyAsync(out_ids, idx->out_ids.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipMemcpyAsync(out_scores, idx->out_scores.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    return VROD_OK;
}


extern "C++" {   // (templates, inside the C entry points' block)
// What setting or getting a range of a row column (labels, tags, values, keys) starts with, in this order; the caller
// returns early on n == 0.  `ptr`: the words to set or the place for the words got; for_set: a set is refused on a
// composite handle and needs an idle one, a get reads the host mirror and needs neither.
static int check_column_args(vrod_index* idx, const char* what, const char* noun, const void* ptr, uint64_t first_id, uint64_t n, bool for_set) {
    if (!idx || (!ptr && n)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    if (for_set) {
        if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "%s on a multi-device handle: %s are not routed to the shards", what, noun);
        VROD_TRY(require_idle(idx, what));
    }
    return check_id_range(idx, first_id, n);
}
// rows [r0, r0 + n) of a checked range take src[0 .. n); the first set of the handle makes the column
template <typename T>
static int column_write(vrod_index* idx, RowColumn<T>& col, uint64_t r0, const T* src, uint64_t n) {
    if (!n) return VROD_OK;
    VROD_TRY(set_device(idx));
    if (!col.exists()) VROD_TRY(col.create(idx->capacity));
    return col.set(r0, src, n);
}
template <typename T>
static int column_set(vrod_index* idx, RowColumn<T>& col, const char* what, uint64_t first_id, const T* src, uint64_t n) {
    VROD_TRY(check_column_args(idx, what, col.noun, src, first_id, n, true));
    return column_write(idx, col, first_id - idx->id_offset, src, n);
}
template <typename T>
static int column_get(vrod_index* idx, const RowColumn<T>& col, uint64_t first_id, uint64_t n, T* out) {
    VROD_TRY(check_column_args(idx, nullptr, nullptr, out, first_id, n, false));
    for (uint64_t i = 0; i < n; ++i) out[i] = col.get(first_id - idx->id_offset + i);   // (the host mirror is the truth)
    return VROD_OK;
}
}  // extern "C++"

int vrod_index_set_labels(vrod_index* idx, uint64_t first_id, const uint32_t* labels, uint64_t n) {
    VROD_TRY(check_column_args(idx, "vrod_index_set_labels", "labels", labels, first_id, n, true));
    if (n) idx->doc_valid = false;
    return column_write(idx, idx->labels, first_id - idx->id_offset, labels, n);
}

int vrod_index_get_labels(vrod_index* idx, uint64_t first_id, uint64_t n, uint32_t* out_labels) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "null argument");
    return column_get(idx, idx->labels, first_id, n, out_labels);
}

static_assert(sizeof(vrod_tag_pred) == 24 && sizeof(TagPred) == 24, "vrod_tag_pred is three packed 64-bit words");
static_assert(sizeof(vrod_where) == 40 && sizeof(WherePred) == 40, "vrod_where is five packed 64-bit words");

// The two forms of a search over groups of rows (S: LabelSearch, TagSearch, WhereSearch; ApiPred: the header's type of
// S::Pred's layout).
static const char kValuesNotRouted[] = "tags and values are not routed to the shards";
extern "C++" {
template <typename S, typename ApiPred>
static int pred_search_host(vrod_index* idx, const char* what, const char* why_not, const float* queries, uint32_t nq, uint32_t k,
                            const ApiPred* preds, uint64_t* out_ids, float* out_scores) {
    VROD_TRY(check_derived_args(idx, what, why_not, nq, {queries, out_ids, out_scores}, true, k, {preds}));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_host_form(idx, what, idx->count ? queries : nullptr, nq, nq, k));   // (an empty handle reads none)
    VROD_TRY(pred_search<S>(idx, idx->host_q.as<float>(), nq, k, reinterpret_cast<const typename S::Pred*>(preds), idx->out_ids.as<uint64_t>(),
                            idx->out_scores.as<float>()));
    return copy_topk_out(idx, nq, k, out_ids, out_scores);
}
template <typename S, typename ApiPred>
static int pred_search_device(vrod_index* idx, const char* what, const char* what_device, const char* why_not, const float* d_queries, uint32_t nq,
                              uint32_t k, const ApiPred* d_preds, uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    VROD_TRY(check_derived_args(idx, what, why_not, nq, {d_queries, d_out_ids, d_out_scores}, true, k, {d_preds}));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, what_device, stream));
    std::vector<typename S::Pred> preds(nq);
    HIP_TRY(hipMemcpy(preds.data(), d_preds, (size_t)nq * sizeof(typename S::Pred), hipMemcpyDeviceToHost));
    return pred_search<S>(idx, d_queries, nq, k, preds.data(), d_out_ids, d_out_scores);
}
}  // extern "C++"

int vrod_search_labeled(vrod_index* idx, const float* queries, uint32_t nq, uint32_t k, const uint32_t* query_labels,
                        uint64_t* out_ids, float* out_scores) {
    return pred_search_host<LabelSearch>(idx, "vrod_search_labeled", kLabelsNotRouted, queries, nq, k, query_labels, out_ids, out_scores);
}

int vrod_search_labeled_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_query_labels,
                               uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    return pred_search_device<LabelSearch>(idx, "vrod_search_labeled", "vrod_search_labeled_device", kLabelsNotRouted, d_queries, nq, k,
                                           d_query_labels, d_out_ids, d_out_scores, stream);
}


int vrod_index_set_tags(vrod_index* idx, uint64_t first_id, const uint64_t* tags, uint64_t n) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "null argument");
    return column_set(idx, idx->tags, "vrod_index_set_tags", first_id, tags, n);
}

int vrod_index_get_tags(vrod_index* idx, uint64_t first_id, uint64_t n, uint64_t* out_tags) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "null argument");
    return column_get(idx, idx->tags, first_id, n, out_tags);
}

int vrod_index_set_values(vrod_index* idx, uint64_t first_id, const int64_t* values, uint64_t n) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "null argument");
    return column_set(idx, idx->values, "vrod_index_set_values", first_id, values, n);
}

int vrod_index_get_values(vrod_index* idx, uint64_t first_id, uint64_t n, int64_t* out_values) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "null argument");
    return column_get(idx, idx->values, first_id, n, out_values);
}

// ------------------------------------------------------------------ row keys
static const char kKeysNotRouted[] = "on a multi-device handle: keys are not routed to the shards";

// Rows [r0, r0 + n) of a single-device, idle handle take keys[0 .. n).  checked: the two uniqueness checks run first
// (vrod_index_upsert has made them).  Order: the host check, the device check, every allocation, and only then the
// writes -- the column, then the table: an insert of the range, or, where that could cross the load limit, one rebuild
// from the column, which holds the new keys by then.
static int keys_set_range(vrod_index* idx, const char* what, uint64_t r0, const uint64_t* keys, uint64_t n, bool checked) {
    const uint32_t* del = idx->del_bits.data();
    std::vector<uint64_t> live_keys;   // what the live rows of the range get
    uint64_t had = 0;                  // ... and how many of them hold a key now
    for (uint64_t i = 0; i < n; ++i) {
        if (bit_of(del, r0 + i)) continue;
        if (keys[i] != kKeyNone) live_keys.push_back(keys[i]);
        if (idx->keys.exists()) had += idx->keys.host[r0 + i] != kKeyNone;
    }
    const uint64_t incoming = live_keys.size();
    VROD_TRY(set_device(idx));
    if (checked) {
        std::sort(live_keys.begin(), live_keys.end());
        const auto twice = std::adjacent_find(live_keys.begin(), live_keys.end());
        if (twice != live_keys.end())
            return fail(VROD_ERR_INVALID_ARG, "%s: key %llu is given to two live rows", what, (unsigned long long)*twice);
        if (idx->ktab.slot_key && incoming) {
            VROD_TRY(idx->host_args.ensure(n * 8));
            HIP_TRY(hipMemcpyAsync(idx->host_args.p, keys, n * 8, hipMemcpyHostToDevice, idx->stream));
            HIP_TRY(hipMemsetAsync(key_ctr(idx), 0, sizeof(KeyCounters), idx->stream));
            launch_keys_check(idx->ktab, idx->keys.d(), idx->del_dev.p, idx->count, idx->host_args.as<uint64_t>(), r0, n, key_ctr(idx), idx->stream);
            HIP_TRY(hipGetLastError());
            KeyCounters c{};
            VROD_TRY(keys_take_counters(idx, what, c));
            if (c.err & kKeyErrHeld) return fail(VROD_ERR_INVALID_ARG, "%s: a key is held by a live row outside the range", what);
        }
    }
    const bool first = !idx->ktab.slot_key;
    const bool rebuild = first || key_needs_rebuild(idx->key_occupied, incoming, idx->ktab.slots);
    const uint64_t sized_for = idx->keyed_live + incoming;   // the live keyed rows plus the incoming keys
    if (rebuild) VROD_TRY(keys_table_clear(idx, sized_for));
    VROD_TRY(column_write(idx, idx->keys, r0, keys, n));
    idx->keyed_live = idx->keyed_live - had + incoming;
    if (rebuild) return keys_rebuild(idx, sized_for, !first, what);
    return keys_insert(idx, r0, n, what);
}

int vrod_index_set_keys(vrod_index* idx, uint64_t first_id, const uint64_t* keys, uint64_t n) {
    VROD_TRY(check_column_args(idx, "vrod_index_set_keys", "keys", keys, first_id, n, true));
    if (!n) return VROD_OK;
    return keys_set_range(idx, "vrod_index_set_keys", first_id - idx->id_offset, keys, n, true);
}

int vrod_index_get_keys(vrod_index* idx, uint64_t first_id, uint64_t n, uint64_t* out_keys) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "null argument");
    return column_get(idx, idx->keys, first_id, n, out_keys);
}

// what the four lookups start with; a null pointer is fine while n == 0
static int check_lookup_args(vrod_index* idx, const char* what, const void* in, uint64_t n, const void* out) {
    if (!idx || ((!in || !out) && n)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "%s %s", what, kKeysNotRouted);
    return require_idle(idx, what);
}

// d_keys[0, n) -> d_out_ids, on the handle's stream, complete on return.  A handle without keys answers with a fill.
static int keys_find_on_device(vrod_index* idx, const char* what, const uint64_t* d_keys, uint64_t n, uint64_t* d_out_ids) {
    hipStream_t s = idx->stream;
    if (!idx->keys.exists()) {
        HIP_TRY(hipMemsetAsync(d_out_ids, 0xFF, n * 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return VROD_OK;
    }
    HIP_TRY(hipMemsetAsync(key_ctr(idx), 0, sizeof(KeyCounters), s));
    launch_keys_find(idx->ktab, idx->keys.d(), idx->del_dev.p, idx->count, idx->id_offset, d_keys, n, d_out_ids, key_ctr(idx), s);
    HIP_TRY(hipGetLastError());
    KeyCounters c{};
    VROD_TRY(keys_take_counters(idx, what, c));
    static const bool report = [] { const char* e = getenv("VROD_DEBUG_KEYS_WALK"); return e && e[0] == '1'; }();
    if (report)   // slots visited per key, one line on stderr (scripts/probes/keys_probe.py)
        fprintf(stderr, "{\"vrod_keys_find\": %llu, \"slots_visited\": %llu, \"slots\": %llu, \"occupied\": %llu}\n", (unsigned long long)n,
                c.find_walk, (unsigned long long)idx->ktab.slots, (unsigned long long)idx->key_occupied);
    return VROD_OK;
}

// the host form's body, also the first step of vrod_index_delete_keys and vrod_index_upsert
static int keys_find_host(vrod_index* idx, const char* what, const uint64_t* keys, uint64_t n, uint64_t* out_ids) {
    if (!idx->keys.exists()) { std::fill(out_ids, out_ids + n, (uint64_t)kKeyNone); return VROD_OK; }
    VROD_TRY(set_device(idx));
    VROD_TRY(idx->host_args.ensure(n * 8));
    VROD_TRY(idx->out_ids.ensure(n * 8));
    HIP_TRY(hipMemcpyAsync(idx->host_args.p, keys, n * 8, hipMemcpyHostToDevice, idx->stream));
    VROD_TRY(keys_find_on_device(idx, what, idx->host_args.as<uint64_t>(), n, idx->out_ids.as<uint64_t>()));
    HIP_TRY(hipMemcpy(out_ids, idx->out_ids.p, n * 8, hipMemcpyDeviceToHost));
    return VROD_OK;
}

int vrod_index_find_keys(vrod_index* idx, const uint64_t* keys, uint64_t n, uint64_t* out_ids) {
    VROD_TRY(check_lookup_args(idx, "vrod_index_find_keys", keys, n, out_ids));
    if (!n) return VROD_OK;
    return keys_find_host(idx, "vrod_index_find_keys", keys, n, out_ids);
}

int vrod_index_find_keys_device(vrod_index* idx, const uint64_t* d_keys, uint64_t n, uint64_t* d_out_ids, void* stream) {
    VROD_TRY(check_lookup_args(idx, "vrod_index_find_keys_device", d_keys, n, d_out_ids));
    if (!n) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_index_find_keys_device", stream));
    return keys_find_on_device(idx, "vrod_index_find_keys_device", d_keys, n, d_out_ids);
}

int vrod_index_ids_to_keys(vrod_index* idx, const uint64_t* ids, uint64_t n, uint64_t* out_keys) {
    VROD_TRY(check_lookup_args(idx, "vrod_index_ids_to_keys", ids, n, out_keys));
    for (uint64_t i = 0; i < n; ++i) {   // the host mirror is the truth
        const bool row = idx->keys.exists() && ids[i] != kKeyNone && ids[i] >= idx->id_offset && ids[i] - idx->id_offset < idx->count;
        out_keys[i] = row ? idx->keys.host[ids[i] - idx->id_offset] : (uint64_t)kKeyNone;
    }
    return VROD_OK;
}

int vrod_index_ids_to_keys_device(vrod_index* idx, const uint64_t* d_ids, uint64_t n, uint64_t* d_out_keys, void* stream) {
    VROD_TRY(check_lookup_args(idx, "vrod_index_ids_to_keys_device", d_ids, n, d_out_keys));
    if (!n) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_index_ids_to_keys_device", stream));
    if (!idx->keys.exists()) HIP_TRY(hipMemsetAsync(d_out_keys, 0xFF, n * 8, idx->stream));
    else launch_keys_translate(idx->keys.d(), idx->count, idx->id_offset, d_ids, n, d_out_keys, idx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(idx->stream));
    return VROD_OK;
}

int vrod_index_delete_keys(vrod_index* idx, const uint64_t* keys, uint64_t n, uint64_t* out_deleted) {
    if (out_deleted) *out_deleted = 0;
    VROD_TRY(check_lookup_args(idx, "vrod_index_delete_keys", keys, n, keys));
    if (!n) return VROD_OK;
    std::vector<uint64_t> rows(n);
    VROD_TRY(keys_find_host(idx, "vrod_index_delete_keys", keys, n, rows.data()));
    rows.erase(std::remove(rows.begin(), rows.end(), (uint64_t)kKeyNone), rows.end());   // lists kept outside outlive deletes
    for (uint64_t& r : rows) r -= idx->id_offset;
    const uint64_t before = idx->n_deleted;
    if (!rows.empty()) VROD_TRY(index_delete_rows(idx, rows));   // (a key named twice found one row: deleting again is a no-op)
    if (out_deleted) *out_deleted = idx->n_deleted - before;
    return VROD_OK;
}

// vrod_index_upsert on an idle single-device handle, n > 0; keys and out_ids: host memory.  The held and the new rows are
// taken from the source through lists of them.
static int upsert_checked(vrod_index* idx, const uint64_t* keys, const RowSource& src, uint64_t n, uint64_t* out_ids) {
    // every check before the first row is written: the keys on the host, the vectors by a prepare-only pass
    {
        std::vector<uint64_t> sorted(keys, keys + n);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() == kKeyNone) return fail(VROD_ERR_INVALID_ARG, "vrod_index_upsert: VROD_ID_NONE is not a key");
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end()) return fail(VROD_ERR_INVALID_ARG, "vrod_index_upsert: key %llu is named twice", (unsigned long long)*twice);
    }
    VROD_TRY(index_update_pass(idx, nullptr, src, n, false));
    std::vector<uint64_t> found(n);
    VROD_TRY(keys_find_host(idx, "vrod_index_upsert", keys, n, found.data()));
    // the rows of held keys are updated in place, the others appended in the order of the call and keyed
    std::vector<uint32_t> dst;
    std::vector<uint64_t> new_keys;
    std::vector<uint64_t> held_pick, new_pick;
    const uint64_t count0 = idx->count;
    for (uint64_t i = 0; i < n; ++i) {
        if (found[i] != kKeyNone) {
            dst.push_back((uint32_t)(found[i] - idx->id_offset));
            held_pick.push_back(i);
        } else {
            found[i] = idx->id_offset + count0 + new_keys.size();
            new_keys.push_back(keys[i]);
            new_pick.push_back(i);
        }
    }
    if (!new_keys.empty()) {
        VROD_TRY(index_add(idx, rows_picked(src, new_pick.data()), new_keys.size()));
        VROD_TRY(keys_set_range(idx, "vrod_index_upsert", count0, new_keys.data(), new_keys.size(), false));
    }
    if (!dst.empty()) VROD_TRY(index_update(idx, dst, rows_picked(src, held_pick.data()), dst.size()));
    if (out_ids) std::copy(found.begin(), found.end(), out_ids);
    return VROD_OK;
}

int vrod_index_upsert(vrod_index* idx, const uint64_t* keys, const float* rows, uint64_t n, uint64_t* out_ids) {
    if (!idx || ((!keys || !rows) && n)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "vrod_index_upsert %s", kKeysNotRouted);
    VROD_TRY(require_idle(idx, "vrod_index_upsert"));
    if (!n) return VROD_OK;
    return upsert_checked(idx, keys, rows_on_host(rows, idx->dim), n, out_ids);
}

int vrod_index_upsert_device(vrod_index* idx, const uint64_t* d_keys, const void* d_rows, int src_dtype, uint64_t row_stride, uint64_t n,
                             uint64_t* d_out_ids, void* stream) {
    VROD_TRY(check_ingest_args(idx, "vrod_index_upsert_device", d_rows, src_dtype, row_stride, n));
    if (!d_keys && n) return fail(VROD_ERR_INVALID_ARG, "vrod_index_upsert_device: d_keys is null");
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "vrod_index_upsert_device %s", kKeysNotRouted);
    VROD_TRY(require_idle(idx, "vrod_index_upsert_device"));
    if (!n) return VROD_OK;
    RowSource src = rows_on_device(d_rows, src_dtype, row_stride);
    VROD_TRY(ingest_open(idx, "vrod_index_upsert_device", d_rows, stream, &src.device));
    std::vector<uint64_t> keys(n), ids(n);   // the keys cross to the host for the host form's checks; the rows stay
    HIP_TRY(hipMemcpy(keys.data(), d_keys, n * 8, hipMemcpyDeviceToHost));
    VROD_TRY(upsert_checked(idx, keys.data(), src, n, ids.data()));
    if (d_out_ids) HIP_TRY(hipMemcpy(d_out_ids, ids.data(), n * 8, hipMemcpyHostToDevice));
    return VROD_OK;
}

int vrod_index_key_stats(const vrod_index* idx, vrod_key_stats* out) {
    if (!idx || !out) return fail(VROD_ERR_INVALID_ARG, "null argument");
    out->keyed_live = idx->keyed_live;
    out->slots = idx->ktab.slots;
    out->occupied = idx->key_occupied;
    out->rebuilds = idx->key_rebuilds;
    out->max_probe = idx->key_max_probe;
    return VROD_OK;
}

int vrod_search_tagged(vrod_index* idx, const float* queries, uint32_t nq, uint32_t k, const vrod_tag_pred* preds, uint64_t* out_ids,
                       float* out_scores) {
    return pred_search_host<TagSearch>(idx, "vrod_search_tagged", kTagsNotRouted, queries, nq, k, preds, out_ids, out_scores);
}

int vrod_search_tagged_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const vrod_tag_pred* d_preds,
                              uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    return pred_search_device<TagSearch>(idx, "vrod_search_tagged", "vrod_search_tagged_device", kTagsNotRouted, d_queries, nq, k, d_preds,
                                         d_out_ids, d_out_scores, stream);
}

int vrod_search_where(vrod_index* idx, const float* queries, uint32_t nq, uint32_t k, const vrod_where* preds, uint64_t* out_ids,
                      float* out_scores) {
    return pred_search_host<WhereSearch>(idx, "vrod_search_where", kValuesNotRouted, queries, nq, k, preds, out_ids, out_scores);
}

int vrod_search_where_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const vrod_where* d_preds, uint64_t* d_out_ids,
                             float* d_out_scores, void* stream) {
    return pred_search_device<WhereSearch>(idx, "vrod_search_where", "vrod_search_where_device", kValuesNotRouted, d_queries, nq, k, d_preds,
                                           d_out_ids, d_out_scores, stream);
}

// ------------------------------------------------------------------ row predicates (vrod_index_*_where)
// A predicate over a row's tags, value and label as an operation on the rows: count, select, delete, filter, retag.  The
// columns stay on the device (kernels_rowpred.hip); what a mutation brings to the host is ONE BIT PER ROW, the hit
// bitmap, from which the mirrors are updated by the steps the id-based calls use: commit_fresh_deletes for a delete,
// index_set_filter for a filter.  Workspaces, the handle being idle: lab_tab [table | totals], lab_cnt the per-group
// counts, lab_mask the hit bitmap, out_ids a host form's selection.
static_assert(sizeof(vrod_row_pred) == 48 && sizeof(RowPred) == 48 && offsetof(vrod_row_pred, label) == 40 && offsetof(RowPred, has_label) == 44,
              "vrod_row_pred is five packed 64-bit words and two 32-bit ones");
static_assert(kRowPredRowsPerGroup % 64 == 0 && kRowTile % 64 == 0, "a hit bitmap of whole waves lies within capacity / 32 words");

// What the six entry points refuse before they look at the handle's state, then the handle's own refusals, in this order:
// a null handle or pointer (preds, and every pointer of `needed`), unknown flag bits, has_label beyond 1, a multi-device
// handle, a pending search.
static int check_rowpred_args(vrod_index* idx, const char* what, const vrod_row_pred* preds, uint32_t n_preds, uint32_t flags,
                              std::initializer_list<const void*> needed, uint32_t known_flags = VROD_ROWPRED_ALLOWED) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    if (n_preds && !preds) return fail(VROD_ERR_INVALID_ARG, "%s: null predicate", what);
    for (const void* p : needed)
        if (!p) return fail(VROD_ERR_INVALID_ARG, "%s: null argument", what);
    if (flags & ~known_flags) return fail(VROD_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", what, flags);
    for (uint32_t i = 0; i < n_preds; ++i)
        if (preds[i].has_label > 1u) return fail(VROD_ERR_INVALID_ARG, "%s: has_label is %u in predicate %u, not 0 or 1", what, preds[i].has_label, i);
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "%s on a multi-device handle: labels, tags and values are not routed to the shards", what);
    return require_idle(idx, what);
}

// The header's struct as the kernels take it; a label that is not compared is 0, so equal predicates have equal bytes.
static RowPred row_pred_of(const vrod_row_pred& p) { return RowPred{p.any, p.all, p.none, p.lo, p.hi, p.has_label ? p.label : 0u, p.has_label}; }

// Bit set = the row is out of an operation's scope: the deleted rows, and under VROD_ROWPRED_ALLOWED the rows the filter
// does not allow (the effective mask holds both).  Null: every row below the count is in scope.
static const uint32_t* rowpred_scope(const vrod_index* idx, uint32_t flags) {
    if ((flags & VROD_ROWPRED_ALLOWED) && idx->filter_on) return idx->eff_dev.p;
    return idx->n_deleted ? idx->del_dev.p : nullptr;
}

// One predicate's hit bitmap over rows [0, count), count > 0, into lab_mask on the handle's stream; counted: each
// work-group's hits into lab_cnt as well, one word more than the groups (the total's place).
static int rowpred_hits(vrod_index* idx, const RowPred& p, const uint32_t* scope, bool counted) {
    VROD_TRY(set_device(idx));
    VROD_TRY(idx->lab_mask.ensure(row_pred_hit_words(idx->count) * 4));
    if (counted) VROD_TRY(idx->lab_cnt.ensure(((size_t)row_pred_groups(idx->count) + 1) * 4));
    launch_rowpred_hits(idx->tags.d(), idx->values.d(), idx->labels.d(), scope, idx->count, p, idx->lab_mask.as<uint32_t>(),
                        counted ? idx->lab_cnt.as<uint32_t>() : nullptr, idx->stream);
    HIP_TRY(hipGetLastError());
    return VROD_OK;
}
// ... and brought to the host: the one bit per row that crosses
static int rowpred_hits_to_host(vrod_index* idx, std::vector<uint32_t>& bits) {
    bits.resize(row_pred_hit_words(idx->count));
    HIP_TRY(hipMemcpyAsync(bits.data(), idx->lab_mask.p, bits.size() * 4, hipMemcpyDeviceToHost, idx->stream));
    HIP_TRY(hipStreamSynchronize(idx->stream));
    return VROD_OK;
}

int vrod_index_count_where(vrod_index* idx, const vrod_row_pred* preds, uint32_t n_preds, uint32_t flags, uint64_t* out_counts) {
    VROD_TRY(check_rowpred_args(idx, "vrod_index_count_where", preds, n_preds, flags, {n_preds ? (const void*)out_counts : (const void*)idx}));
    if (!n_preds) return VROD_OK;
    // the distinct satisfiable predicates, in the table's order; slot[i]: where preds[i] is counted
    std::vector<RowPred> all(n_preds), table;
    std::vector<uint32_t> order, slot(n_preds, UINT32_MAX);
    for (uint32_t i = 0; i < n_preds; ++i) {
        all[i] = row_pred_of(preds[i]);
        if (!row_pred_unsatisfiable(all[i])) order.push_back(i);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return row_pred_before(all[a], all[b]); });
    for (uint32_t i : order) {
        if (table.empty() || row_pred_before(table.back(), all[i])) table.push_back(all[i]);
        slot[i] = (uint32_t)table.size() - 1;
    }
    std::vector<uint32_t> totals(table.size(), 0u);
    if (idx->count && !table.empty()) {
        VROD_TRY(set_device(idx));
        hipStream_t s = idx->stream;
        const uint32_t n_groups = row_pred_groups(idx->count), Gc = (uint32_t)std::min<size_t>(table.size(), kRowPredsPerPass);
        VROD_TRY(idx->lab_tab.ensure((size_t)Gc * (sizeof(RowPred) + 4)));
        VROD_TRY(idx->lab_cnt.ensure((size_t)n_groups * Gc * 4));
        RowPred* d_table = idx->lab_tab.as<RowPred>();
        uint32_t* d_total = (uint32_t*)(d_table + Gc);
        const uint32_t* scope = rowpred_scope(idx, flags);
        for (size_t c0 = 0; c0 < table.size(); c0 += kRowPredsPerPass) {   // one pass over the columns per table
            const uint32_t Gp = (uint32_t)std::min<size_t>(kRowPredsPerPass, table.size() - c0);
            HIP_TRY(hipMemcpyAsync(d_table, table.data() + c0, (size_t)Gp * sizeof(RowPred), hipMemcpyHostToDevice, s));
            launch_pred_group_count(rows_of<RowPredRows>(idx), scope, idx->count, kRowPredRowsPerGroup, d_table, Gp, idx->lab_cnt.as<uint32_t>(), Gp, s);
            launch_group_prefix(idx->lab_cnt.as<uint32_t>(), n_groups, Gp, d_total, s);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(totals.data() + c0, d_total, (size_t)Gp * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    for (uint32_t i = 0; i < n_preds; ++i) out_counts[i] = slot[i] == UINT32_MAX ? 0ull : totals[slot[i]];
    return VROD_OK;
}

// Both forms of vrod_index_select_where behind their checks.  d_out: where the ids go on the device (the caller's
// memory, or null for the host form, which takes the handle's out_ids and copies to h_out).
static int rowpred_select(vrod_index* idx, const char* what, const vrod_row_pred* pred, uint32_t flags, uint64_t capacity, uint64_t* out_count,
                          uint64_t* d_out, uint64_t* h_out) {
    const RowPred p = row_pred_of(*pred);
    uint32_t total = 0;
    hipStream_t s = idx->stream;
    const bool pass = idx->count && !row_pred_unsatisfiable(p);
    uint32_t* d_first = nullptr;
    if (pass) {
        VROD_TRY(rowpred_hits(idx, p, rowpred_scope(idx, flags), true));
        const uint32_t n_groups = row_pred_groups(idx->count);
        d_first = idx->lab_cnt.as<uint32_t>();
        launch_group_prefix(d_first, n_groups, 1, d_first + n_groups, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&total, d_first + n_groups, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *out_count = total;
    if (total > capacity)
        return fail(VROD_ERR_CAPACITY, "%s: %u matching rows, capacity %llu", what, total, (unsigned long long)capacity);
    if (!total) return VROD_OK;
    if (!d_out) {
        VROD_TRY(idx->out_ids.ensure((size_t)total * 8));
        d_out = idx->out_ids.as<uint64_t>();
    }
    launch_rowpred_scatter(idx->lab_mask.as<uint32_t>(), idx->count, d_first, idx->id_offset, d_out, s);
    HIP_TRY(hipGetLastError());
    if (h_out) HIP_TRY(hipMemcpyAsync(h_out, d_out, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VROD_OK;
}

int vrod_index_select_where(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, uint64_t capacity, uint64_t* out_count,
                            uint64_t* out_ids) {
    VROD_TRY(check_rowpred_args(idx, "vrod_index_select_where", pred, 1, flags, {pred, out_count, capacity ? (const void*)out_ids : (const void*)pred}));
    return rowpred_select(idx, "vrod_index_select_where", pred, flags, capacity, out_count, nullptr, out_ids);
}

int vrod_index_select_where_device(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, uint64_t capacity, uint64_t* out_count,
                                   uint64_t* d_out_ids, void* stream) {
    VROD_TRY(check_rowpred_args(idx, "vrod_index_select_where_device", pred, 1, flags,
                                {pred, out_count, capacity ? (const void*)d_out_ids : (const void*)pred}));
    VROD_TRY(begin_sync_device(idx, "vrod_index_select_where_device", stream));
    return rowpred_select(idx, "vrod_index_select_where_device", pred, flags, capacity, out_count, d_out_ids, nullptr);
}

int vrod_index_delete_where(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, uint64_t* out_deleted) {
    VROD_TRY(check_rowpred_args(idx, "vrod_index_delete_where", pred, 1, flags, {pred}));
    const RowPred p = row_pred_of(*pred);
    uint64_t died = 0;
    if (idx->count && !row_pred_unsatisfiable(p)) {
        std::vector<uint32_t> bits;
        VROD_TRY(rowpred_hits(idx, p, rowpred_scope(idx, flags), false));
        VROD_TRY(rowpred_hits_to_host(idx, bits));
        VROD_TRY(index_delete_hits(idx, bits.data(), bits.size(), &died));
    }
    if (out_deleted) *out_deleted = died;
    return VROD_OK;
}

int vrod_index_set_filter_where(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags) {
    VROD_TRY(check_rowpred_args(idx, "vrod_index_set_filter_where", pred, 1, flags, {pred}));
    const RowPred p = row_pred_of(*pred);
    // the allow bits of rows [0, count): a row's bit says whether it matches, deleted or not
    std::vector<uint32_t> bits(std::max<uint64_t>(row_pred_hit_words(idx->count), 1), 0u);
    if (idx->count && !row_pred_unsatisfiable(p)) {
        VROD_TRY(rowpred_hits(idx, p, nullptr, false));
        VROD_TRY(rowpred_hits_to_host(idx, bits));
    }
    if ((flags & VROD_ROWPRED_ALLOWED) && idx->filter_on)   // narrow the filter that is set: what it allows AND matches
        for (size_t w = 0; w < bits.size(); ++w) bits[w] &= w < idx->allow_bits.size() ? idx->allow_bits[w] : 0u;
    return index_set_filter(idx, bits.data(), idx->count);
}

int vrod_index_set_tags_where(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, uint64_t set_bits, uint64_t clear_bits,
                              uint64_t* out_changed) {
    if (idx && (set_bits & clear_bits)) return fail(VROD_ERR_INVALID_ARG, "vrod_index_set_tags_where: set_bits and clear_bits share bits");
    VROD_TRY(check_rowpred_args(idx, "vrod_index_set_tags_where", pred, 1, flags, {pred}));
    const RowPred p = row_pred_of(*pred);
    uint64_t changed = 0;
    // without a column every row carries 0: clearing bits changes nothing, and nothing is allocated
    const bool may_change = set_bits || (clear_bits && idx->tags.exists());
    if (idx->count && !row_pred_unsatisfiable(p) && may_change) {
        VROD_TRY(set_device(idx));
        VROD_TRY(idx->lab_mask.ensure(row_pred_hit_words(idx->count) * 4));
        if (!idx->tags.exists()) {   // as the first set_tags makes it (its clear runs on the null stream: drained before ours reads)
            VROD_TRY(idx->tags.create(idx->capacity));
            HIP_TRY(hipStreamSynchronize(nullptr));
        }
        std::vector<uint32_t> bits;
        launch_rowpred_retag(idx->tags.d(), idx->values.d(), idx->labels.d(), rowpred_scope(idx, flags), idx->count, p, set_bits, clear_bits,
                             idx->lab_mask.as<uint32_t>(), idx->stream);
        int rc = hipGetLastError() == hipSuccess ? rowpred_hits_to_host(idx, bits) : fail(VROD_ERR_HIP, "vrod_index_set_tags_where: the launch failed");
        if (rc != VROD_OK) {   // the mirror is the truth: the device column goes back to it
            (void)hipStreamSynchronize(idx->stream);
            (void)hipMemcpy(idx->tags.d(), idx->tags.host.data(), idx->count * 8, hipMemcpyHostToDevice);
            return rc;
        }
        for (size_t w = 0; w < bits.size(); ++w)   // the changed rows' masks in the mirror
            for (uint32_t b = bits[w]; b; b &= b - 1u) {
                uint64_t& t = idx->tags.host[w * 32 + (size_t)__builtin_ctz(b)];
                t = (t & ~clear_bits) | set_bits;
                ++changed;
            }
    }
    if (out_changed) *out_changed = changed;
    return VROD_OK;
}

// ------------------------------------------------------------------ ordered selection (vrod_index_select_ordered)
// The top `limit` rows by (value, id) among the rows select_where lists, after a keyset cursor (order_plan.h,
// kernels_order.hip, DESIGN.md "Ordered selection"): a filter pass, a radix select when the rows after the cursor exceed
// the limit, a collect pass and a sort, all on the handle's stream.  The host waits twice: for the total, which decides
// whether the select runs and how many records the sort gets, and for the outputs.  Workspaces, the handle being idle:
// lab_mask the hit bitmap, lab_cnt the groups' hit counts, ord_ws, ord_rec, and out_ids / out_scores for a host form's
// ids and values.
static_assert(sizeof(vrod_order_cursor) == 16 && offsetof(vrod_order_cursor, id) == 8, "vrod_order_cursor is two packed 64-bit words");
static_assert(VROD_MAX_ORDERED == kOrderMaxRows && sizeof(OrderState) == 16, "the header's limit is the sort's; the state is 16 bytes");

// Both forms behind their checks.  d_ids / d_vals: where ids and values go on the device (the caller's memory, or the
// handle's for the host form, which copies to h_ids / h_vals); d_vals null: no values are wanted.
static int order_select(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, const vrod_order_cursor* after, uint32_t limit,
                        uint64_t* out_count, uint64_t* out_total, uint64_t* d_ids, int64_t* d_vals, uint64_t* h_ids, int64_t* h_vals) {
    const RowPred p = row_pred_of(*pred);
    const bool desc = (flags & VROD_ORDER_DESC) != 0;
    uint32_t total = 0;
    hipStream_t s = idx->stream;
    const uint32_t n_groups = row_pred_groups(idx->count);
    if (idx->count && !row_pred_unsatisfiable(p)) {
        VROD_TRY(set_device(idx));
        VROD_TRY(idx->lab_mask.ensure(row_pred_hit_words(idx->count) * 4));
        VROD_TRY(idx->lab_cnt.ensure(((size_t)n_groups + 1) * 4));
        uint32_t* d_first = idx->lab_cnt.as<uint32_t>();
        launch_order_hits(idx->tags.d(), idx->values.d(), idx->labels.d(), rowpred_scope(idx, flags), idx->count, p, desc, after != nullptr,
                          after ? order_key(after->value, desc) : 0ull, after ? after->id : 0ull, idx->id_offset, idx->lab_mask.as<uint32_t>(),
                          d_first, s);
        launch_group_prefix(d_first, n_groups, 1, d_first + n_groups, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&total, d_first + n_groups, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    const uint32_t n = std::min(limit, total);
    if (n) {
        const size_t hist_bytes = (size_t)kOrderRounds * kOrderBins * 4;
        VROD_TRY(idx->ord_ws.ensure(hist_bytes + sizeof(OrderState) + ((size_t)n_groups * 2 + 2) * 4));
        VROD_TRY(idx->ord_rec.ensure((size_t)order_sort_size(n) * 16));
        if (!d_ids) {
            VROD_TRY(idx->out_ids.ensure((size_t)n * 8));
            d_ids = idx->out_ids.as<uint64_t>();
            if (h_vals) {
                VROD_TRY(idx->out_scores.ensure((size_t)n * 8));
                d_vals = idx->out_scores.as<int64_t>();
            }
        }
        uint32_t* d_hist = idx->ord_ws.as<uint32_t>();
        OrderState* d_state = (OrderState*)((char*)idx->ord_ws.p + hist_bytes);
        uint32_t* d_cnt2 = (uint32_t*)(d_state + 1);
        const uint32_t* d_hits = idx->lab_mask.as<uint32_t>();
        const bool take_all = total <= limit;
        if (!take_all) launch_order_select(d_hits, idx->values.d(), idx->count, desc, limit, d_hist, d_state, s);
        launch_order_collect(d_hits, idx->values.d(), idx->count, desc, idx->id_offset, take_all, d_state, d_cnt2, idx->lab_cnt.as<uint32_t>(),
                             idx->ord_rec.as<uint64_t>(), n, s);
        launch_order_sort(idx->ord_rec.as<uint64_t>(), n, desc, d_ids, d_vals, s);
        HIP_TRY(hipGetLastError());
        if (h_ids) HIP_TRY(hipMemcpyAsync(h_ids, d_ids, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        if (h_vals) HIP_TRY(hipMemcpyAsync(h_vals, d_vals, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *out_count = n;
    if (out_total) *out_total = total;
    return VROD_OK;
}

static int check_order_args(vrod_index* idx, const char* what, const vrod_row_pred* pred, uint32_t flags, uint32_t limit,
                            const uint64_t* out_count, const uint64_t* out_ids) {
    if (idx && limit > VROD_MAX_ORDERED) return fail(VROD_ERR_INVALID_ARG, "%s: limit must be in 0..%u", what, VROD_MAX_ORDERED);
    return check_rowpred_args(idx, what, pred, 1, flags, {pred, out_count, limit ? (const void*)out_ids : (const void*)pred},
                              VROD_ROWPRED_ALLOWED | VROD_ORDER_DESC);
}

int vrod_index_select_ordered(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, const vrod_order_cursor* after, uint32_t limit,
                              uint64_t* out_count, uint64_t* out_total, uint64_t* out_ids, int64_t* out_values) {
    VROD_TRY(check_order_args(idx, "vrod_index_select_ordered", pred, flags, limit, out_count, out_ids));
    return order_select(idx, pred, flags, after, limit, out_count, out_total, nullptr, nullptr, out_ids, out_values);
}

int vrod_index_select_ordered_device(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, const vrod_order_cursor* after, uint32_t limit,
                                     uint64_t* out_count, uint64_t* out_total, uint64_t* d_out_ids, int64_t* d_out_values, void* stream) {
    VROD_TRY(check_order_args(idx, "vrod_index_select_ordered_device", pred, flags, limit, out_count, d_out_ids));
    VROD_TRY(begin_sync_device(idx, "vrod_index_select_ordered_device", stream));
    return order_select(idx, pred, flags, after, limit, out_count, out_total, d_out_ids, d_out_values, nullptr, nullptr);
}

// ------------------------------------------------------------------ row aggregation (vrod_index_aggregate_where)
// Count, min / max / sum of the value and the smallest id of every group among the rows select_where lists, the groups
// being labels, value buckets or tag bits (aggregate_plan.h, kernels_aggregate.hip, DESIGN.md "Row aggregation"): a
// reset of the table, the aggregation pass and a compaction of the occupied slots, all on the handle's stream.  The host
// waits twice: for the counters, which say whether the call failed and how many records to make room for, and for the
// records.  Only the groups cross to the host, where they are ordered: at most 48 MiB, and a sort of records the caller
// is about to read anyway.  Workspaces, the handle being idle: agg_tab and agg_out.
static_assert(sizeof(vrod_agg_group) == 48 && sizeof(AggGroup) == 48 && offsetof(vrod_agg_group, count) == 8 &&
                  offsetof(vrod_agg_group, sum_value) == 32 && offsetof(vrod_agg_group, first_id) == 40 && offsetof(AggGroup, first_id) == 40,
              "vrod_agg_group is six packed 64-bit words");
static_assert(VROD_MAX_AGG_GROUPS == kAggMaxGroups && VROD_AGG_BY_LABEL == kAggByLabel && VROD_AGG_BY_VALUE == kAggByValue &&
                  VROD_AGG_BY_TAG == kAggByTag && VROD_AGG_ORDER_COUNT == kAggOrderCount,
              "the header's constants are the plan's");

int vrod_index_aggregate_where(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, uint32_t by, int64_t width, uint32_t limit,
                               uint64_t* out_count, uint64_t* out_groups, uint64_t* out_rows, vrod_agg_group* out) {
    const char* what = "vrod_index_aggregate_where";
    if (idx && by > VROD_AGG_BY_TAG) return fail(VROD_ERR_INVALID_ARG, "%s: by is %u, not 0, 1 or 2", what, by);
    if (idx && by == VROD_AGG_BY_VALUE && width < 1) return fail(VROD_ERR_INVALID_ARG, "%s: width must be at least 1", what);
    VROD_TRY(check_rowpred_args(idx, what, pred, 1, flags, {pred, out_count, limit ? (const void*)out : (const void*)pred},
                                VROD_ROWPRED_ALLOWED | VROD_AGG_ORDER_COUNT));
    const RowPred p = row_pred_of(*pred);
    AggCounters ctr{};
    std::vector<AggGroup> groups;
    if (idx->count && !row_pred_unsatisfiable(p)) {
        VROD_TRY(set_device(idx));
        hipStream_t s = idx->stream;
        const bool direct = by == VROD_AGG_BY_TAG;
        const uint64_t slots = direct ? kAggTagGroups : agg_table_slots(idx->count);
        VROD_TRY(idx->agg_tab.ensure(agg_table_bytes(slots)));
        const AggTable tab = agg_table_view(idx->agg_tab.p, slots);
        // the columns the predicate and the mode read; the value is always aggregated
        const bool need_tags = direct || p.any || p.all || p.none, need_labels = by == VROD_AGG_BY_LABEL || p.has_label;
        launch_agg_reset(tab, direct, s);
        launch_agg_pass(by, need_tags ? idx->tags.d() : nullptr, idx->values.d(), need_labels ? idx->labels.d() : nullptr,
                        rowpred_scope(idx, flags), idx->count, p, by == VROD_AGG_BY_VALUE ? width : 1, idx->id_offset, tab, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&ctr, tab.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (ctr.err & kAggErrGroups)
            return fail(VROD_ERR_CAPACITY, "%s: more than %u distinct groups", what, VROD_MAX_AGG_GROUPS);
        if (ctr.err) return fail(VROD_ERR_INTERNAL, "%s: the group table overflowed (%llu slots)", what, (unsigned long long)slots);
        // every claimed slot and the marker key's own may hold a group
        const uint64_t room = limit ? (direct ? kAggTagGroups : ctr.claimed + 1) : 0;
        if (room) VROD_TRY(idx->agg_out.ensure((size_t)room * sizeof(AggGroup)));
        launch_agg_compact(tab, room ? idx->agg_out.as<AggGroup>() : nullptr, room, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&ctr.n_out, &tab.ctr->n_out, 8, hipMemcpyDeviceToHost, s));
        groups.resize(room);   // at most one record more than there are groups
        if (room) HIP_TRY(hipMemcpyAsync(groups.data(), idx->agg_out.p, (size_t)room * sizeof(AggGroup), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (ctr.n_out > VROD_MAX_AGG_GROUPS)   // exactly the cap in hashed slots, and the marker key's group beside them
            return fail(VROD_ERR_CAPACITY, "%s: more than %u distinct groups", what, VROD_MAX_AGG_GROUPS);
        if (room) {
            if (ctr.n_out > room) return fail(VROD_ERR_INTERNAL, "%s: %llu groups, room for %llu", what, (unsigned long long)ctr.n_out, (unsigned long long)room);
            groups.resize(ctr.n_out);
            if (flags & VROD_AGG_ORDER_COUNT) std::sort(groups.begin(), groups.end(), agg_before_count);
            else std::sort(groups.begin(), groups.end(), agg_before_key);
        }
    }
    const uint64_t n = std::min<uint64_t>(limit, ctr.n_out);
    if (n) memcpy(out, groups.data(), (size_t)n * sizeof(AggGroup));
    *out_count = n;
    if (out_groups) *out_groups = ctr.n_out;
    if (out_rows) *out_rows = ctr.rows;
    return VROD_OK;
}

// ------------------------------------------------------------------ group centroids (vrod_index_centroids_where)
// The exact vector sum or mean of every group (centroid_plan.h, kernels_centroid.hip, DESIGN.md "Group centroids"), all
// on the handle's stream: the aggregation above gives the groups, their counts and their table; the host orders them and
// uploads keys and counts; a launch turns the table into slot -> rank; on L2 and IP handles a max pass gives the scale;
// the accumulators are zeroed, the add pass reads every considered row once, and a finishing launch writes the floats.
// The host waits for the counters, for the records, and (L2, IP) for the max word.  Every refusal -- the capacity and a
// non-finite element included -- comes before the first write to the caller's memory.
static_assert(sizeof(vrod_centroid_group) == 24 && sizeof(CentroidGroup) == 24 && offsetof(vrod_centroid_group, count) == 8 &&
                  offsetof(vrod_centroid_group, first_id) == 16 && offsetof(CentroidGroup, first_id) == 16,
              "vrod_centroid_group is three packed 64-bit words");
static_assert(VROD_CENTROID_SUM == kCentroidSum && VROD_MAX_CENTROID_GROUPS == kCentroidMaxGroups && kCentroidMaxGroups <= kAggMaxGroups,
              "the header's constants are the plan's");

// What both forms refuse, in this order: a null handle, an unknown key, a bad width, then check_rowpred_args (null
// pointers, flag bits, has_label, a multi-device handle, a pending search), then the capacity and the stride.
static int check_centroid_args(vrod_index* idx, const char* what, const vrod_row_pred* pred, uint32_t flags, uint32_t by, int64_t width,
                               uint32_t capacity, const uint64_t* out_count, const vrod_centroid_group* out_groups, const float* vectors,
                               uint64_t stride) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "%s: idx is null", what);
    if (by > VROD_AGG_BY_VALUE) return fail(VROD_ERR_INVALID_ARG, "%s: by is %u, not VROD_AGG_BY_LABEL or VROD_AGG_BY_VALUE", what, by);
    if (by == VROD_AGG_BY_VALUE && width < 1) return fail(VROD_ERR_INVALID_ARG, "%s: width must be at least 1", what);
    VROD_TRY(check_rowpred_args(idx, what, pred, 1, flags, {pred, out_count, out_groups, vectors}, VROD_ROWPRED_ALLOWED | VROD_CENTROID_SUM));
    if (capacity == 0 || capacity > VROD_MAX_CENTROID_GROUPS)
        return fail(VROD_ERR_INVALID_ARG, "%s: capacity must be in 1..%u", what, VROD_MAX_CENTROID_GROUPS);
    if (stride < idx->dim) return fail(VROD_ERR_INVALID_ARG, "%s: out_row_stride %llu is less than dim %u", what, (unsigned long long)stride, idx->dim);
    if (stride > UINT64_MAX / capacity) return fail(VROD_ERR_INVALID_ARG, "%s: capacity * out_row_stride overflows", what);
    return VROD_OK;
}

// Both forms behind their checks.  The vectors go to d_out (device memory on out_device, the device form) or to h_out.
static int centroids_where(vrod_index* idx, const char* what, const vrod_row_pred* pred, uint32_t flags, uint32_t by, int64_t width, uint32_t capacity,
                           uint64_t* out_count, uint64_t* out_rows, vrod_centroid_group* out_groups, float* d_out, int out_device, float* h_out,
                           uint64_t stride) {
    const RowPred p = row_pred_of(*pred);
    AggCounters ctr{};
    std::vector<AggGroup> groups;
    if (idx->count && !row_pred_unsatisfiable(p)) {
        VROD_TRY(set_device(idx));
        hipStream_t s = idx->stream;
        const uint32_t dim = idx->dim;
        const uint64_t slots = agg_table_slots(idx->count);
        VROD_TRY(idx->agg_tab.ensure(agg_table_bytes(slots)));
        const AggTable tab = agg_table_view(idx->agg_tab.p, slots);
        const bool need_tags = p.any || p.all || p.none, need_labels = by == VROD_AGG_BY_LABEL || p.has_label;
        const uint32_t* scope = rowpred_scope(idx, flags);
        const int64_t w = by == VROD_AGG_BY_VALUE ? width : 1;
        // 1. the groups and their counts
        launch_agg_reset(tab, false, s);
        launch_agg_pass(by, need_tags ? idx->tags.d() : nullptr, idx->values.d(), need_labels ? idx->labels.d() : nullptr, scope, idx->count, p, w,
                        idx->id_offset, tab, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&ctr, tab.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // 2. the capacity: every claimed slot holds a group (the marker key's may hold one more)
        if ((ctr.err & kAggErrGroups) || ctr.claimed > capacity)
            return fail(VROD_ERR_CAPACITY, "%s: more than %u groups", what, capacity);
        if (ctr.err) return fail(VROD_ERR_INTERNAL, "%s: the group table overflowed (%llu slots)", what, (unsigned long long)slots);
        const uint64_t room = ctr.claimed + 1;
        VROD_TRY(idx->agg_out.ensure((size_t)room * sizeof(AggGroup)));
        launch_agg_compact(tab, idx->agg_out.as<AggGroup>(), room, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&ctr.n_out, &tab.ctr->n_out, 8, hipMemcpyDeviceToHost, s));
        groups.resize(room);
        HIP_TRY(hipMemcpyAsync(groups.data(), idx->agg_out.p, (size_t)room * sizeof(AggGroup), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (ctr.n_out > room) return fail(VROD_ERR_INTERNAL, "%s: %llu groups, room for %llu", what, (unsigned long long)ctr.n_out, (unsigned long long)room);
        if (ctr.n_out > capacity) return fail(VROD_ERR_CAPACITY, "%s: %llu groups, capacity %u", what, (unsigned long long)ctr.n_out, capacity);
        groups.resize(ctr.n_out);
        const uint32_t G = (uint32_t)ctr.n_out;
        if (G) {
            // 3. the order, and the table's slots as ranks
            std::sort(groups.begin(), groups.end(), agg_before_key);
            std::vector<uint64_t> up((size_t)G * 2);   // [keys | counts], as centroid_ws_view lays them out
            for (uint32_t g = 0; g < G; ++g) { up[g] = (uint64_t)groups[g].key; up[(size_t)G + g] = groups[g].count; }
            VROD_TRY(idx->cen_ws.ensure(centroid_ws_bytes(G, slots)));
            const CentroidWs ws = centroid_ws_view(idx->cen_ws.p, G);
            HIP_TRY(hipMemsetAsync(ws.max_bits, 0, 8, s));
            HIP_TRY(hipMemcpyAsync(ws.keys, up.data(), up.size() * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(ws.rank, 0xFF, (size_t)(slots + 1) * 4, s));
            launch_centroid_ranks(tab, ws.keys, G, ws.rank, s);
            VROD_TRY(rowpred_hits(idx, p, scope, false));   // the considered rows, a bit each, in lab_mask
            // 4. the scale: fixed under COSINE, from the largest considered element otherwise
            const bool scaled = idx->metric != VROD_METRIC_COSINE;
            uint32_t m = 0;
            if (scaled) launch_centroid_max(idx->corpus.p, idx->dtype, dim, idx->ld, idx->lab_mask.as<uint32_t>(), idx->count, ws.max_bits, s);
            HIP_TRY(hipGetLastError());
            if (scaled) HIP_TRY(hipMemcpyAsync(&m, ws.max_bits, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));   // the max word is here, and the upload has left `up`
            if (m >= kCentroidNonFinite) return fail(VROD_ERR_INVALID_ARG, "%s: a considered row holds an infinity or a NaN", what);
            const int32_t E = scaled ? centroid_exponent(m) : kCentroidCosineExponent;
            const int32_t scale = centroid_scale(centroid_row_bits(idx->count), E);
            // 5. - 7. zeroed accumulators, the add pass, the floats
            VROD_TRY(idx->cen_acc.ensure(centroid_acc_bytes(G, dim)));
            HIP_TRY(hipMemsetAsync(idx->cen_acc.p, 0, centroid_acc_bytes(G, dim), s));
            launch_centroid_add(idx->corpus.p, idx->dtype, dim, idx->ld, idx->lab_mask.as<uint32_t>(), idx->count, by,
                                by == VROD_AGG_BY_VALUE ? idx->values.d() : nullptr, by == VROD_AGG_BY_LABEL ? idx->labels.d() : nullptr, w, tab, ws.rank, G, scale, idx->cen_acc.as<int64_t>(), s);
            HIP_TRY(hipGetLastError());
            const bool sums = flags & VROD_CENTROID_SUM, direct = d_out && out_device == idx->device && !ingest_force_stage();
            if (!direct) VROD_TRY(idx->raw_stage.ensure((size_t)G * dim * 4));
            launch_centroid_finish(idx->cen_acc.as<int64_t>(), ws.counts, G, dim, scale, sums, direct ? d_out : idx->raw_stage.as<float>(),
                                   direct ? stride : dim, s);
            HIP_TRY(hipGetLastError());
            if (!direct)   // dense rows here, then a pitched copy to the host or to the other device
                HIP_TRY(hipMemcpy2DAsync(d_out ? d_out : h_out, (size_t)stride * 4, idx->raw_stage.p, (size_t)dim * 4, (size_t)dim * 4, G,
                                         d_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    for (size_t g = 0; g < groups.size(); ++g) out_groups[g] = vrod_centroid_group{groups[g].key, groups[g].count, groups[g].first_id};
    *out_count = groups.size();
    if (out_rows) *out_rows = ctr.rows;
    return VROD_OK;
}

int vrod_index_centroids_where(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, uint32_t by, int64_t width, uint32_t capacity,
                               uint64_t* out_count, uint64_t* out_rows, vrod_centroid_group* out_groups, float* out_vectors, uint64_t out_row_stride) {
    const char* what = "vrod_index_centroids_where";
    VROD_TRY(check_centroid_args(idx, what, pred, flags, by, width, capacity, out_count, out_groups, out_vectors, out_row_stride));
    return centroids_where(idx, what, pred, flags, by, width, capacity, out_count, out_rows, out_groups, nullptr, 0, out_vectors, out_row_stride);
}

int vrod_index_centroids_where_device(vrod_index* idx, const vrod_row_pred* pred, uint32_t flags, uint32_t by, int64_t width, uint32_t capacity,
                                      uint64_t* out_count, uint64_t* out_rows, vrod_centroid_group* out_groups, float* d_out_vectors,
                                      uint64_t out_row_stride, void* stream) {
    const char* what = "vrod_index_centroids_where_device";
    VROD_TRY(check_centroid_args(idx, what, pred, flags, by, width, capacity, out_count, out_groups, d_out_vectors, out_row_stride));
    if ((uintptr_t)d_out_vectors % 4) return fail(VROD_ERR_INVALID_ARG, "%s: d_out_vectors is not aligned to its element", what);
    int out_device = 0;
    VROD_TRY(ingest_open(idx, what, d_out_vectors, stream, &out_device));
    return centroids_where(idx, what, pred, flags, by, width, capacity, out_count, out_rows, out_groups, d_out_vectors, out_device, nullptr,
                           out_row_stride);
}

// ------------------------------------------------------------------ duplicate rows (vrod_index_find_duplicates, _delete_duplicates)
// The classes of live rows with the same stored bits (dup_plan.h, kernels_dup.hip, DESIGN.md "Duplicate rows"): a hash
// pass over the corpus, a class pass through a table that lives for this call only, an output pass.  What crosses to
// the host is the counters and, in the host form, the map -- for a delete one bit per row, which index_delete_hits turns
// into tombstones as it does for a delete by predicate.  Workspaces, the handle being idle: the call's own block (given
// back on return: 44 to 76 bytes per live row are too much to keep), out_ids for a host form's map, lab_mask for a
// delete's bitmap.
static_assert(sizeof(vrod_dup_stats) == 56 && sizeof(DupCounters) == 32, "seven 64-bit words; the counters keep what follows them 8-byte aligned");
static_assert(kDupEmpty == kScatterSkip && (uint64_t)kDupEmpty > 0xFFFFFF00ull, "no row of a shard is the empty slot's word");

static int check_dup_args(vrod_index* idx, const char* what, uint32_t flags, const void* out_first, uint64_t map_len) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    if (flags & ~(uint32_t)(VROD_DUP_WITHIN_LABEL | VROD_DUP_NARROW_HASH)) return fail(VROD_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", what, flags);
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "%s on a multi-device handle: equal rows may lie on different shards", what);
    VROD_TRY(require_idle(idx, what));
    if (out_first ? map_len != idx->count : map_len != 0)
        return fail(VROD_ERR_INVALID_ARG, "%s: a map of %llu entries for a handle of %llu rows", what, (unsigned long long)map_len, (unsigned long long)idx->count);
    return VROD_OK;
}

// The three passes behind their checks, on the handle's stream, complete on return.  d_out_first (may be null): the map,
// device memory; want_hits: lab_mask gets the bitmap of the live rows that are not their class's first.  Everything that
// can be refused comes before the first write.  *st is written on success only.
static int dup_run(vrod_index* idx, const char* what, uint32_t flags, uint64_t* d_out_first, bool want_hits, vrod_dup_stats* st) {
    const uint64_t count = idx->count, live = idx->live();
    vrod_dup_stats out{};
    VROD_TRY(set_device(idx));
    hipStream_t s = idx->stream;
    if (!live) {   // no class: every row of the map is a deleted row's
        if (d_out_first && count) {
            HIP_TRY(hipMemsetAsync(d_out_first, 0xFF, count * 8, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        *st = out;
        return VROD_OK;
    }
    if (!dup_pitch_ok(idx->dim, (uint32_t)idx->esize, idx->ld)) return fail(VROD_ERR_INTERNAL, "%s: a row pitch of %u elements", what, idx->ld);
    const bool within = (flags & VROD_DUP_WITHIN_LABEL) != 0, narrow = (flags & VROD_DUP_NARROW_HASH) != 0;
    const uint64_t slots = dup_table_slots(live);
    // the call's block: [hash (u64, count) | counters | slot_row (slots) | slot_min (slots) | row_slot (count)]
    const size_t at_ctr = count * 8, at_tab = at_ctr + sizeof(DupCounters), at_rows = at_tab + slots * 8, total = at_rows + count * 4;
    DevMem<> ws;
    HIP_TRY(ws.alloc(total));
    if (want_hits) VROD_TRY(idx->lab_mask.ensure(row_pred_hit_words(count) * 4));
    uint64_t* d_hash = ws.get<uint64_t>();
    DupCounters* d_ctr = (DupCounters*)(ws.get<char>() + at_ctr);
    DupTable T;
    T.slot_row = (uint32_t*)(ws.get<char>() + at_tab);
    T.slot_min = T.slot_row + slots;
    T.row_slot = (uint32_t*)(ws.get<char>() + at_rows);
    T.slots = slots;
    const uint32_t* del = idx->n_deleted ? idx->del_dev.p : nullptr;
    const uint32_t* labels = within ? idx->labels.d() : nullptr;   // (null: every row carries label 0)
    static const bool timed = [] { const char* e = getenv("VROD_DEBUG_DUP_TIMING"); return e && e[0] == '1'; }();
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timed) { HIP_TRY(hipEventCreate(&ev[0])); HIP_TRY(hipEventCreate(&ev[1])); }

    HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(DupCounters), s));
    HIP_TRY(hipMemsetAsync(T.slot_row, 0xFF, slots * 8, s));   // both arrays: empty slots, all-ones minima
    if (timed) HIP_TRY(hipEventRecord(ev[0], s));
    launch_dup_hash(idx->corpus.p, idx->dim, idx->ld, (uint32_t)idx->esize, count, del, labels, within, narrow, d_hash, s);
    if (timed) HIP_TRY(hipEventRecord(ev[1], s));
    launch_dup_class(idx->corpus.p, idx->dim, idx->ld, (uint32_t)idx->esize, count, del, labels, within, d_hash, T, d_ctr, s);
    // the hashes are done with: the first count words of their block count the classes' rows
    HIP_TRY(hipMemsetAsync(d_hash, 0, count * 4, s));
    launch_dup_output(count, del, T, idx->id_offset, d_out_first, (uint32_t*)d_hash, want_hits ? idx->lab_mask.as<uint32_t>() : nullptr, d_ctr, s);
    HIP_TRY(hipGetLastError());
    DupCounters c{};
    HIP_TRY(hipMemcpyAsync(&c, d_ctr, sizeof c, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (timed) {   // one line on stderr (scripts/probes/dup_probe.py)
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        fprintf(stderr, "{\"vrod_dup_hash_ms\": %.6f, \"live\": %llu, \"slots\": %llu}\n", ms, (unsigned long long)live, (unsigned long long)slots);
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
    }
    if (c.err)
        return fail(VROD_ERR_INTERNAL, "%s: the class table's walk failed (%s)", what, c.err & kDupErrFull ? "ran over every slot" : "a slot names no row");
    out.live = live;
    out.classes = c.classes;
    out.duplicates = live - c.classes;
    out.largest_class = c.largest_class;
    out.slots = slots;
    out.max_probe = c.max_probe;
    out.compare_misses = c.compare_misses;
    *st = out;
    return VROD_OK;
}

int vrod_index_find_duplicates(vrod_index* idx, uint32_t flags, uint64_t* out_first, uint64_t map_len, vrod_dup_stats* out_stats) {
    VROD_TRY(check_dup_args(idx, "vrod_index_find_duplicates", flags, out_first, map_len));
    const bool map = out_first && idx->count;
    if (map) VROD_TRY(set_device(idx));
    if (map) VROD_TRY(idx->out_ids.ensure(idx->count * 8));
    vrod_dup_stats st{};
    VROD_TRY(dup_run(idx, "vrod_index_find_duplicates", flags, map ? idx->out_ids.as<uint64_t>() : nullptr, false, &st));
    if (map) HIP_TRY(hipMemcpy(out_first, idx->out_ids.p, idx->count * 8, hipMemcpyDeviceToHost));
    if (out_stats) *out_stats = st;
    return VROD_OK;
}

int vrod_index_find_duplicates_device(vrod_index* idx, uint32_t flags, uint64_t* d_out_first, uint64_t map_len, vrod_dup_stats* out_stats,
                                      void* stream) {
    VROD_TRY(check_dup_args(idx, "vrod_index_find_duplicates_device", flags, d_out_first, map_len));
    VROD_TRY(begin_sync_device(idx, "vrod_index_find_duplicates_device", stream));
    vrod_dup_stats st{};
    VROD_TRY(dup_run(idx, "vrod_index_find_duplicates_device", flags, d_out_first, false, &st));
    if (out_stats) *out_stats = st;
    return VROD_OK;
}

int vrod_index_delete_duplicates(vrod_index* idx, uint32_t flags, uint64_t* out_deleted) {
    VROD_TRY(check_dup_args(idx, "vrod_index_delete_duplicates", flags, nullptr, 0));
    uint64_t died = 0;
    if (idx->live()) {
        vrod_dup_stats st{};
        std::vector<uint32_t> bits;
        VROD_TRY(dup_run(idx, "vrod_index_delete_duplicates", flags, nullptr, true, &st));
        if (st.duplicates) {
            VROD_TRY(rowpred_hits_to_host(idx, bits));
            VROD_TRY(index_delete_hits(idx, bits.data(), bits.size(), &died));
        }
    }
    if (out_deleted) *out_deleted = died;
    return VROD_OK;
}

// ------------------------------------------------------------------ row lookup (vrod_index_find_rows, _add_unique and their _device forms)
// The join between the inputs of a call and the corpus (rowfind_plan.h, kernels_rowfind.hip, DESIGN.md "Row lookup").
// The corpus is hashed once (launch_dup_hash); the call is cut into lookup batches; a batch is prepared into upd_stage as
// an add would store it (ingest_prepare), hashed and classed as a small corpus of its own (launch_dup_hash / _class), and
// the probe pass streams the corpus's hashes through the batch's table.  What crosses to the host is 16 bytes per input
// (RowfindAnswer) and the counters; rowfind_resolve turns them into ids and the list of the batch's new inputs.
// add_unique appends those through index_add(rows_picked(...)) before the next batch is probed, so that a later batch
// finds them in the corpus; find_rows keeps them in a side corpus of the call, probed the same way.  Either way their
// hashes go behind the corpus's, and row count0 + j stands for the call's j-th new input.
// Workspaces, the handle being idle: the call's own blocks (given back on return), upd_stage for a batch's rows,
// raw_stage and ingest_pick inside the ingest.  Everything that can be refused for the inputs' sake comes before the
// first row is written; whatever fails later rolls the appended rows back as index_add does.
static_assert(sizeof(vrod_rowfind_stats) == 64 && sizeof(RowfindAnswer) == 16, "eight 64-bit words; 16 bytes per input for the host");
static_assert(VROD_ROWFIND_NARROW_HASH == kRowfindNarrowHash && VROD_ROWFIND_SMALL_BATCH == kRowfindSmallBatch && VROD_ID_NONE == kRowfindNone,
              "rowfind_plan.h restates the ABI's flags");
constexpr uint32_t kRowfindXn2Word = 11;   // idx->flags.p[11]: the max squared row norm as an add_unique call found it

// What the four entry points check before any device call; the device forms have run check_ingest_args before.
static int check_rowfind_args(vrod_index* idx, const char* what, const void* rows, uint64_t n, uint32_t flags) {
    if (!idx || (!rows && n)) return fail(VROD_ERR_INVALID_ARG, "%s: null argument", what);
    if (!rowfind_flags_ok(flags)) return fail(VROD_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", what, flags);
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "%s on a multi-device handle: equal rows may lie on different shards", what);
    return require_idle(idx, what);
}

// The rows an add_unique call has appended so far go again: what index_add's own rollback does, for the whole call.
static void rowfind_rollback(vrod_index* idx, uint64_t count0) {
    const uint64_t n = idx->count - count0;
    idx->count = count0;
    if (n) {
        (void)hipMemsetAsync((char*)idx->corpus.p + count0 * idx->row_bytes(), 0, n * idx->row_bytes(), idx->stream);
        (void)hipMemsetAsync(idx->xnorm2.p + count0, 0, n * sizeof(float), idx->stream);
    }
    (void)hipMemcpyAsync(idx->max_xn2_bits, &idx->flags.p[kRowfindXn2Word], 4, hipMemcpyDeviceToDevice, idx->stream);
    (void)hipStreamSynchronize(idx->stream);
}

// The call behind its argument checks, n > 0, on the handle's stream, complete on return.  ids [n]: host memory of the
// caller's flow, meaningful on success; *st is written on success only.
static int rowfind_run(vrod_index* idx, const char* what, const RowSource& src, uint64_t n, uint32_t flags, bool append, uint64_t* ids,
                       vrod_rowfind_stats* st) {
    VROD_TRY(set_device(idx));
    hipStream_t s = idx->stream;
    const uint32_t dim = idx->dim, ld = idx->ld, es = (uint32_t)idx->esize;
    const size_t rb = idx->row_bytes();
    if (!dup_pitch_ok(dim, es, ld)) return fail(VROD_ERR_INTERNAL, "%s: a row pitch of %u elements", what, ld);
    const bool narrow = (flags & kRowfindNarrowHash) != 0, small = (flags & kRowfindSmallBatch) != 0;
    const uint64_t count0 = idx->count, B = rowfind_batch_rows(n, dim, small), nb = rowfind_batches(n, dim, small);
    const uint64_t slots_max = rowfind_table_slots(B);
    const bool side = !append && nb > 1;   // find_rows over several batches: the new inputs of earlier batches are kept

    // ---- every allocation.  The call's block: [hash (u64, count0 + n) | batch hash (u64, B) | answers (B) | counters |
    // slot_row, slot_min, found, found_side (slots each) | row_slot (B) | news (B)]
    const size_t at_bhash = (count0 + n) * 8, at_ans = at_bhash + B * 8, at_ctr = at_ans + B * sizeof(RowfindAnswer), at_tab = at_ctr + sizeof(DupCounters),
                 at_rows = at_tab + slots_max * 16, at_news = at_rows + B * 4, total = at_news + B * 4;
    DevMem<> ws, kept;
    HIP_TRY(ws.alloc(total));
    if (side) HIP_TRY(kept.alloc((n - rowfind_batch_count(n, dim, small, nb - 1)) * rb));
    VROD_TRY(idx->upd_stage.ensure(B * rb));
    if (append && count0 + n > idx->capacity)   // the growth of an add of all n, up front: no batch's append can run out of room
        VROD_TRY(index_reserve(idx, idx->capacity ? std::max(count0 + n, idx->capacity + idx->capacity / 2) : count0 + n));
    uint64_t* d_hash = ws.get<uint64_t>();
    uint64_t* d_bhash = (uint64_t*)(ws.get<char>() + at_bhash);
    RowfindAnswer* d_ans = (RowfindAnswer*)(ws.get<char>() + at_ans);
    DupCounters* d_ctr = (DupCounters*)(ws.get<char>() + at_ctr);
    uint32_t* d_tab = (uint32_t*)(ws.get<char>() + at_tab);
    uint32_t* d_news = (uint32_t*)(ws.get<char>() + at_news);
    std::vector<RowfindAnswer> ans(B);
    std::vector<uint32_t> news(B);
    std::vector<uint64_t> new_inputs(n);

    // ---- every input is checked before the first row is written: a call of several batches by a prepare-only pass
    if (nb > 1) VROD_TRY(index_update_pass(idx, nullptr, src, n, false));

    static const bool timed = [] { const char* e = getenv("VROD_DEBUG_ROWFIND_TIMING"); return e && e[0] == '1'; }();
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 4; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_guard{ev};
    if (timed) for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    float hash_ms = 0.f, probe_ms = 0.f;
    double append_ms = 0.0;

    HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(DupCounters), s));
    if (append) HIP_TRY(hipMemcpyAsync(&idx->flags.p[kRowfindXn2Word], idx->max_xn2_bits, 4, hipMemcpyDeviceToDevice, s));
    if (timed) HIP_TRY(hipEventRecord(ev[0], s));
    launch_dup_hash(idx->corpus.p, dim, ld, es, count0, idx->n_deleted ? idx->del_dev.p : nullptr, nullptr, false, narrow, d_hash, s);
    if (timed) HIP_TRY(hipEventRecord(ev[1], s));
    HIP_TRY(hipGetLastError());

    RowfindTotals tot;
    DupCounters c{};
    int rc = VROD_OK;
    auto batch = [&](uint64_t b) -> int {
        const uint64_t i0 = rowfind_batch_first(n, dim, small, b), m = rowfind_batch_count(n, dim, small, b), slots = rowfind_table_slots(m);
        DupTable T;
        T.slot_row = d_tab;
        T.slot_min = d_tab + slots;
        T.row_slot = (uint32_t*)(ws.get<char>() + at_rows);
        T.slots = slots;
        uint32_t* d_found = d_tab + 2 * slots;
        uint32_t* d_found_side = side && tot.fresh ? d_tab + 3 * slots : nullptr;
        VROD_TRY(ingest_prepare(idx, rows_from(src, i0), m, idx->upd_stage.p));
        if (nb == 1) VROD_TRY(check_bad_flag(idx, "rows"));
        HIP_TRY(hipMemsetAsync(d_tab, 0xFF, slots * 16, s));   // empty slots, all-ones minima, nothing found
        launch_dup_hash(idx->upd_stage.p, dim, ld, es, m, nullptr, nullptr, false, narrow, d_bhash, s);
        launch_dup_class(idx->upd_stage.p, dim, ld, es, m, nullptr, nullptr, false, d_bhash, T, d_ctr, s);
        if (timed) HIP_TRY(hipEventRecord(ev[2], s));
        launch_rowfind_probe(idx->corpus.p, dim, ld, es, idx->count, idx->n_deleted ? idx->del_dev.p : nullptr, d_hash, idx->upd_stage.p, (uint32_t)m,
                             d_bhash, T, d_found, d_ctr, s);
        if (timed) HIP_TRY(hipEventRecord(ev[3], s));
        if (d_found_side)
            launch_rowfind_probe(kept.p, dim, ld, es, tot.fresh, nullptr, d_hash + count0, idx->upd_stage.p, (uint32_t)m, d_bhash, T, d_found_side, d_ctr, s);
        launch_rowfind_resolve((uint32_t)m, T, d_found, d_found_side, count0, d_ans, d_ctr, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&c, d_ctr, sizeof c, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(ans.data(), d_ans, m * sizeof(RowfindAnswer), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (timed) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
            probe_ms += ms;
        }
        if (c.err)
            return fail(VROD_ERR_INTERNAL, "%s: a batch table's walk failed (%s)", what, c.err & kDupErrFull ? "ran over every slot" : "a slot names no row");
        const uint64_t fresh0 = tot.fresh;
        const uint64_t k = rowfind_resolve(ans.data(), i0, m, count0, idx->id_offset, append, ids, new_inputs.data(), news.data(), tot);
        if (!k || (!append && b + 1 == nb)) return VROD_OK;   // (the last batch of a lookup has no later batch to tell)
        const auto t0 = std::chrono::steady_clock::now();
        if (append) VROD_TRY(index_add(idx, rows_picked(src, new_inputs.data() + fresh0), k));
        if (timed) append_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (b + 1 == nb) return VROD_OK;
        HIP_TRY(hipMemcpyAsync(d_news, news.data(), k * 4, hipMemcpyHostToDevice, s));
        launch_rowfind_keep(idx->upd_stage.p, ld, es, d_bhash, d_news, (uint32_t)k, side ? kept.get<char>() + fresh0 * rb : nullptr,
                            d_hash + count0 + fresh0, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));   // (news and the stage are free for the next batch)
        return VROD_OK;
    };
    for (uint64_t b = 0; b < nb && rc == VROD_OK; ++b) rc = batch(b);
    if (rc != VROD_OK) {
        if (append) rowfind_rollback(idx, count0);
        return rc;
    }
    if (timed) {   // one line on stderr (scripts/probes/rowfind_probe.py)
        HIP_TRY(hipEventElapsedTime(&hash_ms, ev[0], ev[1]));
        fprintf(stderr, "{\"vrod_rowfind_hash_ms\": %.6f, \"probe_ms\": %.6f, \"append_ms\": %.6f, \"count\": %llu, \"rows\": %llu, \"batches\": %llu}\n", hash_ms,
                probe_ms, append_ms, (unsigned long long)count0, (unsigned long long)n, (unsigned long long)nb);
    }
    vrod_rowfind_stats o{};
    o.rows = n;
    o.found = tot.found;
    o.repeats = tot.repeats;
    o.appended = append ? tot.fresh : 0;
    o.batches = nb;
    o.slots = slots_max;
    o.max_probe = c.max_probe;
    o.compare_misses = c.compare_misses;
    *st = o;
    return VROD_OK;
}

// The host forms' body: the ids go to the caller's array at the end, if there is one.
static int rowfind_host(vrod_index* idx, const char* what, const float* rows, uint64_t n, uint32_t flags, bool append, uint64_t* out_ids,
                        vrod_rowfind_stats* out_stats) {
    VROD_TRY(check_rowfind_args(idx, what, rows, n, flags));
    vrod_rowfind_stats st{};
    if (n) {
        std::vector<uint64_t> ids(n);
        VROD_TRY(rowfind_run(idx, what, rows_on_host(rows, idx->dim), n, flags, append, ids.data(), &st));
        if (out_ids) std::copy(ids.begin(), ids.end(), out_ids);
    }
    if (out_stats) *out_stats = st;
    return VROD_OK;
}

static int rowfind_device(vrod_index* idx, const char* what, const void* d_rows, int src_dtype, uint64_t row_stride, uint64_t n, uint32_t flags,
                          bool append, uint64_t* d_out_ids, vrod_rowfind_stats* out_stats, void* stream) {
    VROD_TRY(check_ingest_args(idx, what, d_rows, src_dtype, row_stride, n));
    VROD_TRY(check_rowfind_args(idx, what, d_rows, n, flags));
    vrod_rowfind_stats st{};
    if (n) {
        RowSource src = rows_on_device(d_rows, src_dtype, row_stride);
        VROD_TRY(ingest_open(idx, what, d_rows, stream, &src.device));
        std::vector<uint64_t> ids(n);
        if (append && d_out_ids) {   // the one thing that can still be refused behind the appends: try the copy's target first
            hipPointerAttribute_t at{};
            if (hipPointerGetAttributes(&at, d_out_ids) != hipSuccess || at.type != hipMemoryTypeDevice) {
                (void)hipGetLastError();
                return fail(VROD_ERR_INVALID_ARG, "%s: d_out_ids is not in device memory", what);
            }
        }
        VROD_TRY(rowfind_run(idx, what, src, n, flags, append, ids.data(), &st));
        if (d_out_ids) HIP_TRY(hipMemcpy(d_out_ids, ids.data(), n * 8, hipMemcpyHostToDevice));
    }
    if (out_stats) *out_stats = st;
    return VROD_OK;
}

int vrod_index_find_rows(vrod_index* idx, const float* rows, uint64_t n, uint32_t flags, uint64_t* out_ids, vrod_rowfind_stats* out_stats) {
    return rowfind_host(idx, "vrod_index_find_rows", rows, n, flags, false, out_ids, out_stats);
}

int vrod_index_find_rows_device(vrod_index* idx, const void* d_rows, int src_dtype, uint64_t row_stride, uint64_t n, uint32_t flags,
                                uint64_t* d_out_ids, vrod_rowfind_stats* out_stats, void* stream) {
    return rowfind_device(idx, "vrod_index_find_rows_device", d_rows, src_dtype, row_stride, n, flags, false, d_out_ids, out_stats, stream);
}

int vrod_index_add_unique(vrod_index* idx, const float* rows, uint64_t n, uint32_t flags, uint64_t* out_ids, vrod_rowfind_stats* out_stats) {
    return rowfind_host(idx, "vrod_index_add_unique", rows, n, flags, true, out_ids, out_stats);
}

int vrod_index_add_unique_device(vrod_index* idx, const void* d_rows, int src_dtype, uint64_t row_stride, uint64_t n, uint32_t flags,
                                 uint64_t* d_out_ids, vrod_rowfind_stats* out_stats, void* stream) {
    return rowfind_device(idx, "vrod_index_add_unique_device", d_rows, src_dtype, row_stride, n, flags, true, d_out_ids, out_stats, stream);
}

// ------------------------------------------------------------------ near-duplicate rows (vrod_index_find_near_duplicates, _delete_near_duplicates)
// The connected components of the threshold graph over the eligible rows (near_plan.h, kernels_near.hip, DESIGN.md
// "Near-duplicate rows"): a self-join of range scans.  The ascending list of eligible rows -- the gather path's, built
// from the mask's host mirror and uploaded once per mask generation -- is cut into batches; a batch's rows are gathered
// out of the corpus as they are stored (launch_byid_gather) and run through range_collect as queries taken as given
// (prep_ovr), all with the one threshold; the batch's pool entries are united in a union-find in device memory.  A batch
// whose exact total exceeds the call's pool is redone as two halves.  After the last batch one pass writes the map, the
// class sizes, the counts and, for a delete, one bit per row, which index_delete_hits turns into tombstones.  Everything
// runs on the stream of the slot the range scans use, so a batch's union pass is ordered before the next batch's scan
// reuses the pool.  Workspaces, the handle being idle: the call's own block (8 bytes per row, given back on return), the
// slot's raw-query buffer, range_pool, out_ids for a host form's map, lab_mask for a delete's bitmap.
static_assert(sizeof(vrod_near_stats) == 64 && sizeof(NearCounters) == 32, "eight 64-bit words; the counters keep what follows them 8-byte aligned");
static_assert(VROD_NEAR_SMALL_POOL == kNearSmallPool, "near_plan.h restates the ABI's flag");

static int check_near_args(vrod_index* idx, const char* what, float threshold, uint32_t flags, const void* out_first, uint64_t map_len) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    if (!near_flags_ok(flags)) return fail(VROD_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", what, flags);
    if (threshold != threshold) return fail(VROD_ERR_INVALID_VALUE, "%s: the threshold is NaN", what);
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "%s on a multi-device handle: stored rows are not gathered across the shards", what);
    VROD_TRY(require_idle(idx, what));
    if (out_first ? map_len != idx->count : map_len != 0)
        return fail(VROD_ERR_INVALID_ARG, "%s: a map of %llu entries for a handle of %llu rows", what, (unsigned long long)map_len, (unsigned long long)idx->count);
    return VROD_OK;
}

// The whole call behind its checks, complete on return.  d_out_first (may be null): the map, device memory; want_hits:
// lab_mask gets the bitmap of the eligible rows that are not their class's smallest.  Nothing of the caller's and
// nothing of the handle's rows is written before the last batch is through.  *st is written on success only.
static int near_run(vrod_index* idx, const char* what, float threshold, uint32_t flags, uint64_t* d_out_first, bool want_hits, vrod_near_stats* st) {
    const uint64_t count = idx->count, elig = idx->eligible();
    vrod_near_stats out{};
    VROD_TRY(set_device(idx));
    Pending& P = next_slot(idx);
    hipStream_t s = P.stream;
    if (!count || !elig) {   // no class: every row of the map is a row that is not eligible
        if (d_out_first && count) {
            HIP_TRY(hipMemsetAsync(d_out_first, 0xFF, count * 8, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        *st = out;
        return VROD_OK;
    }
    const uint32_t batch = near_batch_rows(idx->dtype == VROD_DTYPE_BF16, elig);
    const uint64_t pool = near_pool_entries(elig, (flags & kNearSmallPool) != 0);
    // ---- what can be refused: the row list, the call's block [counters | parent (count) | class sizes (count)], the
    // batch's queries, the pool, a delete's bitmap
    VROD_TRY(gather_list(idx));
    if (idx->list_n != elig) return fail(VROD_ERR_INTERNAL, "%s: the row list holds %llu rows, %llu are eligible", what, (unsigned long long)idx->list_n, (unsigned long long)elig);
    DevMem<> ws;
    HIP_TRY(ws.alloc(sizeof(NearCounters) + count * 8));
    VROD_TRY(P.q_raw.ensure((size_t)batch * idx->dim * 4));
    VROD_TRY(idx->range_pool.ensure((size_t)std::min<uint64_t>(pool, (uint64_t)batch * elig) * sizeof(RangeHit)));
    if (want_hits) VROD_TRY(idx->lab_mask.ensure(row_pred_hit_words(count) * 4));
    NearCounters* d_ctr = ws.get<NearCounters>();
    uint32_t* d_parent = (uint32_t*)(ws.get<char>() + sizeof(NearCounters));
    uint32_t* d_size = d_parent + count;
    const uint32_t* d_list = idx->list_dev.as<uint32_t>();
    const std::vector<float> thr(batch, threshold);

    HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(NearCounters), s));
    launch_near_init(d_parent, d_size, count, s);
    HIP_TRY(hipGetLastError());
    // ---- the batches, in ascending order; a batch that overflowed is replaced by its halves
    std::vector<NearBatch> todo;
    for (uint64_t b = near_n_batches(elig, batch); b-- > 0;) todo.push_back(near_batch(elig, batch, b));
    RangeShardResult R;
    while (!todo.empty()) {
        const NearBatch b = todo.back();
        todo.pop_back();
        launch_byid_gather(idx->corpus.p, idx->dtype, idx->ld, idx->dim, count, idx->id_offset, nullptr, nullptr, d_list + b.first, 0, b.rows,
                           P.q_raw.as<float>(), nullptr, s);   // (the list holds eligible rows below the count)
        HIP_TRY(hipGetLastError());
        idx->prep_ovr = M_L2;   // set for exactly this enqueue: the stored rows are the queries
        const int rc = range_collect(idx, P.q_raw.as<float>(), b.rows, thr.data(), pool, R);
        idx->prep_ovr = -1;
        VROD_TRY(rc);
        out.batches++;
        switch (near_verdict(b, R.total, pool)) {
            case NEAR_FITS: break;
            case NEAR_SPLIT: {
                NearBatch lo, hi;
                near_halves(b, &lo, &hi);
                todo.push_back(hi);
                todo.push_back(lo);
                out.splits++;
                continue;
            }
            default:
                return fail(VROD_ERR_INTERNAL, "%s: one row has %llu hits among %llu eligible rows", what, (unsigned long long)R.total, (unsigned long long)elig);
        }
        launch_near_union(idx->range_pool.as<RangeHit>(), R.stored, d_list + b.first, b.rows, idx->id_offset, count, d_parent, d_ctr, s);
        HIP_TRY(hipGetLastError());
    }
    // ---- the map, the class sizes, the counts
    launch_near_flatten(count, idx->row_mask(), d_parent, idx->id_offset, d_out_first, d_size, want_hits ? idx->lab_mask.as<uint32_t>() : nullptr, d_ctr, s);
    HIP_TRY(hipGetLastError());
    NearCounters c{};
    HIP_TRY(hipMemcpyAsync(&c, d_ctr, sizeof c, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (c.err)
        return fail(VROD_ERR_INTERNAL, "%s: the union-find failed (%s)", what,
                    c.err & kNearErrRow ? "a hit names no row" : c.err & kNearErrWalk ? "a find walk ran out" : "a link ran out of retries");
    if (c.rows != elig) return fail(VROD_ERR_INTERNAL, "%s: %llu rows were looked at, %llu are eligible", what, (unsigned long long)c.rows, (unsigned long long)elig);
    out.rows = elig;
    out.classes = c.classes;
    out.near_duplicates = elig - c.classes;
    out.largest_class = c.largest_class;
    out.hits = c.hits;
    out.pool_entries = pool;
    *st = out;
    return VROD_OK;
}

int vrod_index_find_near_duplicates(vrod_index* idx, float threshold, uint32_t flags, uint64_t* out_first, uint64_t map_len, vrod_near_stats* out_stats) {
    VROD_TRY(check_near_args(idx, "vrod_index_find_near_duplicates", threshold, flags, out_first, map_len));
    const bool map = out_first && idx->count;
    if (map) VROD_TRY(set_device(idx));
    if (map) VROD_TRY(idx->out_ids.ensure(idx->count * 8));
    vrod_near_stats st{};
    VROD_TRY(near_run(idx, "vrod_index_find_near_duplicates", threshold, flags, map ? idx->out_ids.as<uint64_t>() : nullptr, false, &st));
    if (map) HIP_TRY(hipMemcpy(out_first, idx->out_ids.p, idx->count * 8, hipMemcpyDeviceToHost));
    if (out_stats) *out_stats = st;
    return VROD_OK;
}

int vrod_index_find_near_duplicates_device(vrod_index* idx, float threshold, uint32_t flags, uint64_t* d_out_first, uint64_t map_len,
                                           vrod_near_stats* out_stats, void* stream) {
    VROD_TRY(check_near_args(idx, "vrod_index_find_near_duplicates_device", threshold, flags, d_out_first, map_len));
    VROD_TRY(begin_sync_device(idx, "vrod_index_find_near_duplicates_device", stream));
    vrod_near_stats st{};
    VROD_TRY(near_run(idx, "vrod_index_find_near_duplicates_device", threshold, flags, d_out_first, false, &st));
    if (out_stats) *out_stats = st;
    return VROD_OK;
}

int vrod_index_delete_near_duplicates(vrod_index* idx, float threshold, uint32_t flags, uint64_t* out_deleted) {
    VROD_TRY(check_near_args(idx, "vrod_index_delete_near_duplicates", threshold, flags, nullptr, 0));
    uint64_t died = 0;
    if (idx->count && idx->eligible()) {
        vrod_near_stats st{};
        std::vector<uint32_t> bits;
        VROD_TRY(near_run(idx, "vrod_index_delete_near_duplicates", threshold, flags, nullptr, true, &st));
        if (st.near_duplicates) {
            VROD_TRY(rowpred_hits_to_host(idx, bits));
            VROD_TRY(index_delete_hits(idx, bits.data(), bits.size(), &died));
        }
    }
    if (out_deleted) *out_deleted = died;
    return VROD_OK;
}

static int check_grouped_args(vrod_index* idx, const void* q, uint32_t nq, uint32_t k, const void* oi, const void* os) {
    return check_derived_args(idx, "vrod_search_grouped", kLabelsNotRouted, nq, {q, oi, os}, true, k);
}

int vrod_search_grouped(vrod_index* idx, const float* queries, uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_scores,
                        uint32_t* out_labels) {
    VROD_TRY(check_grouped_args(idx, queries, nq, k, out_ids, out_scores));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_host_form(idx, "vrod_search_grouped", queries, nq, nq, k));
    VROD_TRY(idx->out_col.ensure((size_t)nq * k * 4));
    VROD_TRY(grouped_search(idx, idx->host_q.as<float>(), nq, k, idx->out_ids.as<uint64_t>(), idx->out_scores.as<float>(),
                            idx->out_col.as<uint32_t>()));
    VROD_TRY(copy_topk_out(idx, nq, k, out_ids, out_scores));
    if (out_labels) HIP_TRY(hipMemcpy(out_labels, idx->out_col.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    return VROD_OK;
}

int vrod_search_grouped_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                               uint32_t* d_out_labels, void* stream) {
    VROD_TRY(check_grouped_args(idx, d_queries, nq, k, d_out_ids, d_out_scores));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_search_grouped_device", stream));
    if (!d_out_labels) {   // the de-duplication keeps each query's taken labels there
        VROD_TRY(idx->out_col.ensure((size_t)nq * k * 4));
        d_out_labels = idx->out_col.as<uint32_t>();
    }
    return grouped_search(idx, d_queries, nq, k, d_out_ids, d_out_scores, d_out_labels);
}

static int check_multivec_args(vrod_index* idx, const void* v, const void* lims, uint32_t nq, uint32_t k, const void* ol, const void* os) {
    return check_derived_args(idx, "vrod_search_multivec", kLabelsNotRouted, nq, {v, ol, os}, true, k, {lims});
}

static int check_multivec_lims(const uint32_t* lims, uint32_t nq) {
    switch (multivec_check_lims(lims, nq)) {
        case 0: return VROD_OK;
        case 1: return fail(VROD_ERR_INVALID_ARG, "query_lims[0] must be 0");
        case 2: return fail(VROD_ERR_INVALID_ARG, "query_lims must not decrease");
        case 3: return fail(VROD_ERR_INVALID_ARG, "a query without a vector");
        default: return fail(VROD_ERR_INVALID_ARG, "a query with more than %u vectors", VROD_MAX_QUERY_VECTORS);
    }
}

int vrod_search_multivec(vrod_index* idx, const float* vectors, const uint32_t* query_lims, uint32_t nq, uint32_t k, uint32_t* out_labels,
                         float* out_scores, uint32_t* out_found) {
    VROD_TRY(check_multivec_args(idx, vectors, query_lims, nq, k, out_labels, out_scores));
    if (!nq) return VROD_OK;
    VROD_TRY(require_idle(idx, "vrod_search_multivec"));
    VROD_TRY(check_multivec_lims(query_lims, nq));
    VROD_TRY(begin_host_form(idx, "vrod_search_multivec", vectors, query_lims[nq], nq, k));
    VROD_TRY(idx->out_col.ensure((size_t)nq * k * 4));
    VROD_TRY(idx->out_found.ensure((size_t)nq * 4));
    VROD_TRY(multivec_search(idx, idx->host_q.as<float>(), query_lims, nq, k, idx->out_col.as<uint32_t>(), idx->out_scores.as<float>(),
                             idx->out_found.as<uint32_t>()));
    HIP_TRY(hipMemcpy(out_labels, idx->out_col.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_scores, idx->out_scores.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    if (out_found) HIP_TRY(hipMemcpy(out_found, idx->out_found.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return VROD_OK;
}

int vrod_search_multivec_device(vrod_index* idx, const float* d_vectors, const uint32_t* d_query_lims, uint32_t nq, uint32_t k,
                                uint32_t* d_out_labels, float* d_out_scores, uint32_t* d_out_found, void* stream) {
    VROD_TRY(check_multivec_args(idx, d_vectors, d_query_lims, nq, k, d_out_labels, d_out_scores));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_search_multivec_device", stream));
    std::vector<uint32_t> lims;
    VROD_TRY(read_lims(d_query_lims, nq, lims));
    VROD_TRY(check_multivec_lims(lims.data(), nq));
    if (!d_out_found) {
        VROD_TRY(idx->out_found.ensure((size_t)nq * 4));
        d_out_found = idx->out_found.as<uint32_t>();
    }
    return multivec_search(idx, d_vectors, lims.data(), nq, k, d_out_labels, d_out_scores, d_out_found);
}

int vrod_index_last_multivec(const vrod_index* idx, vrod_multivec_stats* out) {
    if (!idx || !out) return fail(VROD_ERR_INVALID_ARG, "null argument");
    *out = idx->mv_stats;
    return VROD_OK;
}

static int check_diverse_args(vrod_index* idx, const void* q, uint32_t nq, uint32_t k, uint32_t pool, float lambda, const void* oi,
                              const void* os) {
    // (what the arguments alone decide comes first: it is checked, and tested, without a handle)
    switch (diverse_check_args(k, pool, lambda)) {
        case 0: break;
        case 1: return fail(VROD_ERR_INVALID_ARG, "k must be at least 1");
        case 2: return fail(VROD_ERR_INVALID_ARG, "k = %u is larger than the pool, %u", k, pool);
        case 3: return fail(VROD_ERR_INVALID_ARG, "pool must be at most %u", VROD_MAX_DIVERSE_POOL);
        default: return fail(VROD_ERR_INVALID_ARG, "lambda must be in [0, 1]");
    }
    return check_derived_args(idx, "vrod_search_diverse", kRowsNotGathered, nq, {q, oi, os}, false, 0);
}

int vrod_search_diverse(vrod_index* idx, const float* queries, uint32_t nq, uint32_t k, uint32_t pool, float lambda, uint64_t* out_ids,
                        float* out_scores, float* out_mmr) {
    VROD_TRY(check_diverse_args(idx, queries, nq, k, pool, lambda, out_ids, out_scores));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_host_form(idx, "vrod_search_diverse", queries, nq, nq, k));
    VROD_TRY(idx->out_col.ensure((size_t)nq * k * 4));
    VROD_TRY(diverse_search(idx, idx->host_q.as<float>(), nq, k, pool, lambda, idx->out_ids.as<uint64_t>(), idx->out_scores.as<float>(),
                            idx->out_col.as<float>()));
    VROD_TRY(copy_topk_out(idx, nq, k, out_ids, out_scores));
    if (out_mmr) HIP_TRY(hipMemcpy(out_mmr, idx->out_col.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    return VROD_OK;
}

int vrod_search_diverse_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k, uint32_t pool, float lambda,
                               uint64_t* d_out_ids, float* d_out_scores, float* d_out_mmr, void* stream) {
    VROD_TRY(check_diverse_args(idx, d_queries, nq, k, pool, lambda, d_out_ids, d_out_scores));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_search_diverse_device", stream));
    return diverse_search(idx, d_queries, nq, k, pool, lambda, d_out_ids, d_out_scores, d_out_mmr);
}

static int check_byid_args(vrod_index* idx, const void* ids, uint32_t nq, uint32_t k, uint32_t flags, const void* oi, const void* os,
                           const char* what) {
    // (what the arguments alone decide comes first: it is checked, and tested, without a handle)
    if (flags & ~(uint32_t)VROD_BYID_EXCLUDE_SELF) return fail(VROD_ERR_INVALID_ARG, "unknown flag bits 0x%x", flags);
    if (!byid_k_ok(k, flags & VROD_BYID_EXCLUDE_SELF))
        return fail(VROD_ERR_INVALID_ARG, "k must be in 1..%u (1..%u with the self drop)", VROD_MAX_K, VROD_MAX_K - 1);
    return check_derived_args(idx, what, kRowsNotGathered, nq, {ids, oi, os}, false, 0);
}

int vrod_search_by_ids(vrod_index* idx, const uint64_t* ids, uint32_t nq, uint32_t k, uint32_t flags, uint64_t* out_ids, float* out_scores) {
    VROD_TRY(check_byid_args(idx, ids, nq, k, flags, out_ids, out_scores, "vrod_search_by_ids"));
    if (!nq) return VROD_OK;
    VROD_TRY(require_idle(idx, "vrod_search_by_ids"));
    for (uint32_t q = 0; q < nq; ++q) VROD_TRY(check_live_id(idx, ids[q], "id"));
    VROD_TRY(begin_host_form(idx, "vrod_search_by_ids", nullptr, 0, nq, k));
    VROD_TRY(idx->host_args.ensure((size_t)nq * 8));
    HIP_TRY(hipMemcpy(idx->host_args.p, ids, (size_t)nq * 8, hipMemcpyHostToDevice));
    VROD_TRY(byid_search(idx, idx->host_args.as<uint64_t>(), true, nq, k, flags & VROD_BYID_EXCLUDE_SELF, idx->out_ids.as<uint64_t>(),
                         idx->out_scores.as<float>()));
    return copy_topk_out(idx, nq, k, out_ids, out_scores);
}

int vrod_search_by_ids_device(vrod_index* idx, const uint64_t* d_ids, uint32_t nq, uint32_t k, uint32_t flags, uint64_t* d_out_ids,
                              float* d_out_scores, void* stream) {
    VROD_TRY(check_byid_args(idx, d_ids, nq, k, flags, d_out_ids, d_out_scores, "vrod_search_by_ids_device"));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_search_by_ids_device", stream));
    return byid_search(idx, d_ids, false, nq, k, flags & VROD_BYID_EXCLUDE_SELF, d_out_ids, d_out_scores);
}

// What the arguments alone decide comes first (checked, and tested, without a handle), then the handle and the pointers.
static int check_combined_args(vrod_index* idx, const void* term_lims, uint32_t nq, uint32_t k, uint32_t flags, const void* oi, const void* os,
                               const char* what) {
    switch (combine_check_args(k, flags)) {
        case 0: break;
        case 1: return fail(VROD_ERR_INVALID_ARG, "unknown flag bits 0x%x", flags);
        default: return fail(VROD_ERR_INVALID_ARG, "k must be in 1..%u", VROD_MAX_K);
    }
    return check_derived_args(idx, what, kRowsNotGathered, nq, {term_lims, oi, os}, false, 0);
}

// The two lims arrays (host copies; excl_lims may be null) against combine_plan.h, and the pointers their totals require.
static int check_combined_batch(const uint32_t* term_lims, const void* term_ids, const void* term_weights, const uint32_t* excl_lims,
                                const void* excl_ids, bool has_vector, uint32_t nq, uint32_t k, uint32_t flags, CombineCounts* counts) {
    uint32_t q = 0;
    switch (combine_check_batch(term_lims, excl_lims, nq, has_vector, k, flags, counts, &q)) {
        case 0: break;
        case 3: return fail(VROD_ERR_INVALID_ARG, "term_lims must start at 0 and never decrease");
        case 4: return fail(VROD_ERR_INVALID_ARG, "exclude_lims must start at 0 and never decrease");
        case 5: return fail(VROD_ERR_INVALID_ARG, "query %u has no operand: no vector and no term", q);
        case 6: return fail(VROD_ERR_INVALID_ARG, "query %u has more than %u terms", q, VROD_MAX_COMBINE_TERMS);
        case 7: return fail(VROD_ERR_INVALID_ARG, "query %u excludes more than %u ids (its terms included under the flag)", q, VROD_MAX_EXCLUDE);
        default: return fail(VROD_ERR_INVALID_ARG, "k + the largest excluded count must be at most %u", VROD_MAX_K);
    }
    if (term_lims[nq] && (!term_ids || !term_weights)) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    if (excl_lims && excl_lims[nq] && !excl_ids) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    return VROD_OK;
}

int vrod_search_combined(vrod_index* idx, const float* vectors, const float* vector_weights, const uint32_t* term_lims, const uint64_t* term_ids,
                         const float* term_weights, const uint32_t* exclude_lims, const uint64_t* exclude_ids, uint32_t nq, uint32_t k,
                         uint32_t flags, uint64_t* out_ids, float* out_scores) {
    VROD_TRY(check_combined_args(idx, term_lims, nq, k, flags, out_ids, out_scores, "vrod_search_combined"));
    if (!nq) return VROD_OK;
    VROD_TRY(require_idle(idx, "vrod_search_combined"));
    CombineCounts counts;
    VROD_TRY(check_combined_batch(term_lims, term_ids, term_weights, exclude_lims, exclude_ids, vectors != nullptr, nq, k, flags, &counts));
    const uint32_t T = term_lims[nq], X = exclude_lims ? exclude_lims[nq] : 0u;
    for (uint32_t t = 0; t < T; ++t) {
        VROD_TRY(check_live_id(idx, term_ids[t], "term id"));
        if (!std::isfinite(term_weights[t])) return fail(VROD_ERR_INVALID_VALUE, "term weight %u is NaN or Inf", t);
    }
    if (vectors && vector_weights)
        for (uint32_t q = 0; q < nq; ++q)
            if (!std::isfinite(vector_weights[q])) return fail(VROD_ERR_INVALID_VALUE, "vector weight %u is NaN or Inf", q);
    VROD_TRY(begin_host_form(idx, "vrod_search_combined", vectors, vectors ? nq : 0, nq, k));
    // the arguments on the device: [term ids | excluded ids | term weights | vector weights | term lims | exclude lims]
    const bool vw = vectors && vector_weights;
    const size_t o_tid = 0, o_xid = o_tid + (size_t)T * 8, o_tw = o_xid + (size_t)X * 8, o_vw = o_tw + (size_t)T * 4,
                 o_tl = o_vw + (vw ? (size_t)nq * 4 : 0), o_xl = o_tl + ((size_t)nq + 1) * 4, bytes = o_xl + (exclude_lims ? ((size_t)nq + 1) * 4 : 0);
    VROD_TRY(idx->host_args.ensure(bytes));
    char* base = idx->host_args.as<char>();
    if (T) {
        HIP_TRY(hipMemcpy(base + o_tid, term_ids, (size_t)T * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(base + o_tw, term_weights, (size_t)T * 4, hipMemcpyHostToDevice));
    }
    if (X) HIP_TRY(hipMemcpy(base + o_xid, exclude_ids, (size_t)X * 8, hipMemcpyHostToDevice));
    if (vw) HIP_TRY(hipMemcpy(base + o_vw, vector_weights, (size_t)nq * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + o_tl, term_lims, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice));
    if (exclude_lims) HIP_TRY(hipMemcpy(base + o_xl, exclude_lims, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice));
    CombineArgs a{};
    a.d_vectors = vectors ? idx->host_q.as<float>() : nullptr;
    a.d_vector_weights = vw ? (const float*)(base + o_vw) : nullptr;
    a.d_term_lims = (const uint32_t*)(base + o_tl);
    a.d_term_ids = (const uint64_t*)(base + o_tid);
    a.d_term_weights = (const float*)(base + o_tw);
    a.d_excl_lims = exclude_lims ? (const uint32_t*)(base + o_xl) : nullptr;
    a.d_excl_ids = (const uint64_t*)(base + o_xid);
    VROD_TRY(combined_search(idx, a, counts, nq, k, flags, idx->out_ids.as<uint64_t>(), idx->out_scores.as<float>()));
    return copy_topk_out(idx, nq, k, out_ids, out_scores);
}

int vrod_search_combined_device(vrod_index* idx, const float* d_vectors, const float* d_vector_weights, const uint32_t* d_term_lims,
                                const uint64_t* d_term_ids, const float* d_term_weights, const uint32_t* d_exclude_lims,
                                const uint64_t* d_exclude_ids, uint32_t nq, uint32_t k, uint32_t flags, uint64_t* d_out_ids, float* d_out_scores,
                                void* stream) {
    VROD_TRY(check_combined_args(idx, d_term_lims, nq, k, flags, d_out_ids, d_out_scores, "vrod_search_combined_device"));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_search_combined_device", stream));
    std::vector<uint32_t> tl, xl;
    VROD_TRY(read_lims(d_term_lims, nq, tl));
    if (d_exclude_lims) VROD_TRY(read_lims(d_exclude_lims, nq, xl));
    CombineCounts counts;
    VROD_TRY(check_combined_batch(tl.data(), d_term_ids, d_term_weights, d_exclude_lims ? xl.data() : nullptr, d_exclude_ids, d_vectors != nullptr,
                                  nq, k, flags, &counts));
    CombineArgs a{d_vectors, d_vectors ? d_vector_weights : nullptr, d_term_lims, d_term_ids, d_term_weights, d_exclude_lims, d_exclude_ids};
    return combined_search(idx, a, counts, nq, k, flags, d_out_ids, d_out_scores);
}

// The lims array (a host copy) against candidates_plan.h, and the pointers its total requires.
static int check_candidates_lists(const uint32_t* lims, uint32_t nq, const void* ids, const void* out_scores) {
    uint32_t q = 0;
    switch (cand_check_lims(lims, nq, &q)) {
        case 0: break;
        case 1: return fail(VROD_ERR_INVALID_ARG, "cand_lims must start at 0 and never decrease");
        default: return fail(VROD_ERR_INVALID_ARG, "query %u lists more than %u candidates", q, VROD_MAX_CANDIDATES);
    }
    if (lims[nq] && (!ids || !out_scores)) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    return VROD_OK;
}

// A host form's lists on the device: host_args as [ids | lims].
static int upload_candidates(vrod_index* idx, uint32_t nq, const uint32_t* lims, const uint64_t* ids, const uint64_t** d_ids,
                             const uint32_t** d_lims) {
    const size_t n = lims[nq], o_lims = n * 8;
    VROD_TRY(idx->host_args.ensure(o_lims + ((size_t)nq + 1) * 4));
    char* base = idx->host_args.as<char>();
    if (n) HIP_TRY(hipMemcpy(base, ids, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + o_lims, lims, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice));
    *d_ids = (const uint64_t*)base;
    *d_lims = (const uint32_t*)(base + o_lims);
    return VROD_OK;
}

int vrod_search_candidates(vrod_index* idx, const float* queries, uint32_t nq, uint32_t k, const uint32_t* cand_lims, const uint64_t* cand_ids,
                           uint64_t* out_ids, float* out_scores) {
    VROD_TRY(check_derived_args(idx, "vrod_search_candidates", kCandidatesNotRouted, nq, {}, true, k, {queries, cand_lims, out_ids, out_scores}));
    if (!nq) return VROD_OK;
    VROD_TRY(require_idle(idx, "vrod_search_candidates"));
    VROD_TRY(check_candidates_lists(cand_lims, nq, cand_ids, out_scores));
    VROD_TRY(begin_host_form(idx, "vrod_search_candidates", queries, nq, nq, k));
    const uint64_t* d_ids;
    const uint32_t* d_lims;
    VROD_TRY(upload_candidates(idx, nq, cand_lims, cand_ids, &d_ids, &d_lims));
    VROD_TRY(candidates_search(idx, idx->host_q.as<float>(), nq, k, cand_lims, d_lims, d_ids, idx->out_ids.as<uint64_t>(),
                               idx->out_scores.as<float>()));
    return copy_topk_out(idx, nq, k, out_ids, out_scores);
}

int vrod_search_candidates_device(vrod_index* idx, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_cand_lims,
                                  const uint64_t* d_cand_ids, uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    VROD_TRY(check_derived_args(idx, "vrod_search_candidates_device", kCandidatesNotRouted, nq, {}, true, k,
                                {d_queries, d_cand_lims, d_out_ids, d_out_scores}));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_search_candidates_device", stream));
    std::vector<uint32_t> lims;
    VROD_TRY(read_lims(d_cand_lims, nq, lims));
    VROD_TRY(check_candidates_lists(lims.data(), nq, d_cand_ids, d_out_scores));
    return candidates_search(idx, d_queries, nq, k, lims.data(), d_cand_lims, d_cand_ids, d_out_ids, d_out_scores);
}

int vrod_score_candidates(vrod_index* idx, const float* queries, uint32_t nq, const uint32_t* cand_lims, const uint64_t* cand_ids,
                          float* out_scores) {
    VROD_TRY(check_derived_args(idx, "vrod_score_candidates", kCandidatesNotRouted, nq, {}, false, 0, {queries, cand_lims}));
    if (!nq) return VROD_OK;
    VROD_TRY(require_idle(idx, "vrod_score_candidates"));
    VROD_TRY(check_candidates_lists(cand_lims, nq, cand_ids, out_scores));
    VROD_TRY(begin_host_form(idx, "vrod_score_candidates", queries, nq, nq, 0));
    const uint64_t* d_ids;
    const uint32_t* d_lims;
    VROD_TRY(upload_candidates(idx, nq, cand_lims, cand_ids, &d_ids, &d_lims));
    const size_t n = cand_lims[nq];
    VROD_TRY(idx->out_scores.ensure(std::max<size_t>(n, 1) * 4));
    VROD_TRY(candidates_score(idx, idx->host_q.as<float>(), nq, cand_lims, d_lims, d_ids, idx->out_scores.as<float>()));
    if (n) HIP_TRY(hipMemcpy(out_scores, idx->out_scores.p, n * 4, hipMemcpyDeviceToHost));
    return VROD_OK;
}

int vrod_score_candidates_device(vrod_index* idx, const float* d_queries, uint32_t nq, const uint32_t* d_cand_lims, const uint64_t* d_cand_ids,
                                 float* d_out_scores, void* stream) {
    VROD_TRY(check_derived_args(idx, "vrod_score_candidates_device", kCandidatesNotRouted, nq, {}, false, 0, {d_queries, d_cand_lims}));
    if (!nq) return VROD_OK;
    VROD_TRY(begin_sync_device(idx, "vrod_score_candidates_device", stream));
    std::vector<uint32_t> lims;
    VROD_TRY(read_lims(d_cand_lims, nq, lims));
    VROD_TRY(check_candidates_lists(lims.data(), nq, d_cand_ids, d_out_scores));
    return candidates_score(idx, d_queries, nq, lims.data(), d_cand_lims, d_cand_ids, d_out_scores);
}

int vrod_knn_graph(vrod_index* idx, uint64_t first_id, uint64_t n, uint32_t k, uint64_t* out_ids, float* out_scores) {
    VROD_TRY(check_byid_args(idx, (void*)1, n ? 1u : 0u, k, VROD_BYID_EXCLUDE_SELF, out_ids, out_scores, "vrod_knn_graph"));
    VROD_TRY(check_id_range(idx, first_id, n));
    if (!n) return VROD_OK;
    VROD_TRY(require_idle(idx, "vrod_knn_graph"));
    VROD_TRY(set_device(idx));
    return knn_graph(idx, first_id - idx->id_offset, n, k, out_ids, out_scores);
}

int vrod_range_search(vrod_index* idx, const float* queries, uint32_t nq, const float* thresholds, uint64_t capacity,
                      uint64_t* out_lims, uint64_t* out_ids, float* out_scores) {
    VROD_TRY(check_range_args(idx, queries, nq, thresholds, capacity, out_lims, out_ids, out_scores));
    out_lims[0] = 0;
    if (!nq) return VROD_OK;
    VROD_TRY(check_thresholds(thresholds, nq));
    return range_search(idx, queries, true, nq, thresholds, capacity, out_lims, out_ids, out_scores);
}

int vrod_range_search_device(vrod_index* idx, const float* d_queries, uint32_t nq, const float* d_thresholds, uint64_t capacity,
                             uint64_t* d_out_lims, uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    VROD_TRY(check_range_args(idx, d_queries, nq, d_thresholds, capacity, d_out_lims, d_out_ids, d_out_scores));
    // pointers on the handle's (first) device.  The call is synchronous: whatever the caller's stream holds -- the
    // producers of the inputs, the last readers of the outputs -- is complete before the library's streams start.
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    std::vector<uint64_t> lims((size_t)nq + 1, 0);
    std::vector<float> thr(nq);
    int rc = VROD_OK;
    if (nq) {
        HIP_TRY(hipMemcpy(thr.data(), d_thresholds, (size_t)nq * 4, hipMemcpyDeviceToHost));
        VROD_TRY(check_thresholds(thr.data(), nq));
        rc = range_search(idx, d_queries, false, nq, thr.data(), capacity, lims.data(), d_out_ids, d_out_scores);
        if (rc != VROD_OK && rc != VROD_ERR_CAPACITY) return rc;
    }
    const std::string why = g_last_error;
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipMemcpy(d_out_lims, lims.data(), lims.size() * 8, hipMemcpyHostToDevice));
    g_last_error = why;
    return rc;
}

int vrod_merge_topk_device(int device, int metric, const uint64_t* d_ids, const float* d_scores,
                           uint32_t n_lists, uint32_t nq, uint32_t k, uint64_t* d_out_ids,
                           float* d_out_scores, void* stream) {
    if ((nq && k && n_lists) && (!d_ids || !d_scores || !d_out_ids || !d_out_scores)) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    if (!valid_metric(metric)) return fail(VROD_ERR_INVALID_ARG, "bad metric %d", metric);
    HIP_TRY(hipSetDevice(device));
    launch_merge_topk(score_form(metric), d_ids, d_scores, (uint64_t)nq * k, (uint64_t)nq * k, n_lists, nq, k, d_out_ids, d_out_scores, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return VROD_OK;
}

int vrod_merge_topk_packed_device(int device, int metric, const void* d_packed, uint32_t n_lists, uint32_t nq,
                                  uint32_t k, uint64_t* d_out_ids, float* d_out_scores, void* stream) {
    if ((nq && k && n_lists) && (!d_packed || !d_out_ids || !d_out_scores)) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    if (!valid_metric(metric)) return fail(VROD_ERR_INVALID_ARG, "bad metric %d", metric);
    HIP_TRY(hipSetDevice(device));
    // one rank's block = nq*k ids (u64) followed by nq*k scores (f32): 12*nq*k bytes, 8-B aligned
    // as long as nq*k is even; the stride is given in elements of each array
    const uint64_t block_bytes = (uint64_t)nq * k * 12;
    if (block_bytes % 8 != 0) return fail(VROD_ERR_INVALID_ARG, "nq*k must be even for the packed layout");
    const uint64_t* ids = (const uint64_t*)d_packed;
    const float* scores = (const float*)((const char*)d_packed + (uint64_t)nq * k * 8);
    launch_merge_topk(score_form(metric), ids, scores, block_bytes / 8, block_bytes / 4, n_lists, nq, k, d_out_ids, d_out_scores, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return VROD_OK;
}

int vrod_index_save(vrod_index* idx, const char* path) {
    if (!idx || !path || !path[0]) return fail(VROD_ERR_INVALID_ARG, "null argument");
    if (idx->composite()) return fail(VROD_ERR_UNSUPPORTED, "vrod_index_save on a multi-device handle: a snapshot holds one device's rows");
    VROD_TRY(require_idle(idx, "vrod_index_save"));
    const std::string tmp = std::string(path) + ".tmp";
    SnapFd f;
    f.fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (f.fd < 0) return fail(VROD_ERR_IO, "open %s: %s", tmp.c_str(), strerror(errno));
    int rc = snap_save_body(idx, f.fd);
    if (close(f.fd) != 0 && rc == VROD_OK) rc = fail(VROD_ERR_IO, "close %s: %s", tmp.c_str(), strerror(errno));
    f.fd = -1;
    if (rc == VROD_OK && rename(tmp.c_str(), path) != 0) rc = fail(VROD_ERR_IO, "rename %s -> %s: %s", tmp.c_str(), path, strerror(errno));
    if (rc != VROD_OK) (void)unlink(tmp.c_str());   // whatever is at `path` stays as it was
    return rc;
}

int vrod_index_load(vrod_index** out, const char* path, const int* device_ids, int n_devices) {
    if (!out) return fail(VROD_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (!path || !path[0] || n_devices < 0 || (n_devices > 0 && !device_ids)) return fail(VROD_ERR_INVALID_ARG, "null argument or bad device list");
    if (n_devices > 1) return fail(VROD_ERR_UNSUPPORTED, "vrod_index_load onto a multi-device handle: a snapshot holds one device's rows");
    // everything that needs no device, before the first device call
    SnapFd f;
    SnapHeader h;
    VROD_TRY(snap_open(path, f, h));
    VROD_TRY(snap_verify_sections(f.fd, path, h, kSnapHostVerifyBytes));
    VROD_TRY(snap_check_live(f.fd, path, h));
    vrod_index* idx = nullptr;
    VROD_TRY(vrod_index_create(&idx, h.dim, (int)h.dtype, (int)h.metric, device_ids, n_devices));
    const int rc = snap_load_body(idx, f.fd, path, h);
    if (rc != VROD_OK) {
        const std::string why = g_last_error;
        vrod_index_destroy(idx);
        g_last_error = why;
        return rc;
    }
    *out = idx;
    return VROD_OK;
}

int vrod_snapshot_info(const char* path, struct vrod_snapshot_info* out) {
    if (!path || !out) return fail(VROD_ERR_INVALID_ARG, "null argument");
    SnapFd f;
    SnapHeader h;
    VROD_TRY(snap_open(path, f, h));
    out->version = h.version; out->dim = h.dim; out->dtype = h.dtype; out->metric = h.metric;
    out->count = h.count; out->live_count = h.live_count; out->id_offset = h.id_offset; out->file_bytes = h.file_bytes;
    out->has_filter = h.find(SNAP_FILTER) != nullptr;
    out->has_labels = h.find(SNAP_LABELS) != nullptr;
    out->has_tags = h.find(SNAP_TAGS) != nullptr;
    out->has_values = h.find(SNAP_VALUES) != nullptr;
    return VROD_OK;
}

int vrod_snapshot_verify(const char* path) {
    if (!path) return fail(VROD_ERR_INVALID_ARG, "null argument");
    SnapFd f;
    SnapHeader h;
    VROD_TRY(snap_open(path, f, h));
    VROD_TRY(snap_verify_sections(f.fd, path, h, UINT64_MAX));
    return snap_check_live(f.fd, path, h);
}

int vrod_snapshot_checksum(const void* bytes, uint64_t n_bytes, uint64_t first_word, uint64_t* out) {
    if (!out || (!bytes && n_bytes)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    *out = snap_checksum(bytes, n_bytes, first_word);
    return VROD_OK;
}

int vrod_snapshot_checksum_device(int device, const void* d_bytes, uint64_t n_bytes, uint64_t first_word, uint64_t* out, void* stream) {
    if (!out || (!d_bytes && n_bytes)) return fail(VROD_ERR_INVALID_ARG, "null argument");
    if ((uintptr_t)d_bytes % 4) return fail(VROD_ERR_INVALID_ARG, "d_bytes must be 4-byte aligned");
    HIP_TRY(hipSetDevice(device));
    DevBuf sum;
    VROD_TRY(sum.ensure(8));
    HIP_TRY(hipMemsetAsync(sum.p, 0, 8, (hipStream_t)stream));
    launch_snapshot_checksum(d_bytes, n_bytes, first_word, sum.as<uint64_t>(), (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sum.p, 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return VROD_OK;
}

int vrod_index_set_path(vrod_index* idx, int path) {
    if (!idx || path < VROD_PATH_AUTO || path > VROD_PATH_GATHER) return fail(VROD_ERR_INVALID_ARG, "bad path");
    if (!idx->composite()) VROD_TRY(require_idle(idx, "vrod_index_set_path"));
    idx->path = path;
    return VROD_OK;
}

int vrod_index_set_profiling(vrod_index* idx, int on) {
    if (!idx) return fail(VROD_ERR_INVALID_ARG, "idx is null");
    idx->profiling = on < 0 ? 0 : on > 2 ? 2 : on;
    return VROD_OK;
}

int vrod_index_last_stats(const vrod_index* idx, vrod_search_stats* out) {
    if (!idx || !out) return fail(VROD_ERR_INVALID_ARG, "null argument");
    *out = idx->stats;
    return VROD_OK;
}

int vrod_index_shard_stats(const vrod_index* idx, uint32_t shard, int* out_device, vrod_search_stats* out) {
    if (!idx || !out) return fail(VROD_ERR_INVALID_ARG, "null argument");
    const size_t n = idx->composite() ? idx->shards.size() : 1;
    if (shard >= n) return fail(VROD_ERR_INVALID_ARG, "shard %u of a handle with %zu", shard, n);
    const vrod_index* sh = idx->composite() ? idx->shards[shard] : idx;
    *out = sh->stats;
    if (out_device) *out_device = sh->device;
    return VROD_OK;
}

int vrod_synth_rows_device(int device, uint64_t seed, uint64_t first_row, uint64_t n, uint32_t dim,
                           float* d_out, void* stream) {
    if (n && !d_out) return fail(VROD_ERR_INVALID_ARG, "null buffer");
    HIP_TRY(hipSetDevice(device));
    launch_synth_rows(seed, first_row, n, dim, d_out, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return VROD_OK;
}

}  // extern "C"
