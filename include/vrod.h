/*
 * vrod.h -- C ABI of libvrod_hip.so: the MI355X (gfx950) brute-force similarity
 * scan + top-k that hangs under vRod's SEARCHSIMILAR command.
 *
 * Reference interfaces these entry points stand behind (sekulas/vRod @ 2024-10-24;
 * the reference has NO FFI and NO scan -- these are the slots it leaves empty):
 *   vrod_index_create / _destroy   <- the corpus handle `Database` must own
 *                                     (src/database/mod.rs:6-10, "//TODO collections")
 *   vrod_index_add                 <- BulkInsertCommand::execute / InsertCommand::execute
 *                                     (src/command/types.rs:56-80), rows are the
 *                                     Vec<Vec<f32>> of src/utils/embeddings.rs:29
 *   vrod_index_delete              <- the DELETE command CommandBuilder names (src/command/types.rs, builder.rs)
 *   vrod_index_update              <- the UPDATE command (src/command/types.rs:82, builder.rs:53)
 *   vrod_index_compact             <- the REINDEX command (src/command/types.rs:134, builder.rs:73)
 *   vrod_search                    <- SearchSimilarCommand::execute
 *                                     (src/command/types.rs:121-132), built by
 *                                     CommandBuilder::build "SEARCHSIMILAR"
 *                                     (src/command/builder.rs:68-72)
 *   vrod_last_error                <- the thiserror/anyhow surface (src/main.rs:36-42,
 *                                     src/command/builder.rs:10-15): status + message,
 *                                     never a panic or exception across the ABI
 * The Rust-side binding a maintainer would add is in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; every function returns a vrod_status
 * (0 = ok); the caller owns every in/out buffer; the library never keeps a caller
 * pointer after return; calls on one handle must be serialised by the caller
 * (the reference is Rc<RefCell<_>>: single-threaded, src/command/types.rs:10).
 * All host-pointer entry points are synchronous.
 *
 * Semantics (frozen; DESIGN.md "Scan spec"): ids are row indices in insertion order
 * (+ id_offset); COSINE scores are dot products of L2-normalised vectors (higher is
 * better), L2 scores are squared Euclidean distances (lower is better), IP (maximum
 * inner product) scores are dot products of the prepared vectors -- stored as given,
 * bf16-rounded on BF16 handles, never normalised (higher is better); results are
 * best-first, ties broken by smaller id, a NaN score (an IP dot product whose terms
 * overflow to +inf and -inf) ranks last and still carries its row's id; deleted rows are absent (vrod_index_delete);
 * unfilled slots (k > live rows) are (VROD_ID_NONE, NaN).  Results are bit-identical to the CPU oracle
 * (oracle/), except that a NaN score matches any NaN.
 *
 * Environment (read once per process; everything else the library reads is
 * VROD_DEBUG_*: A/B switches of the build's own experiments):
 *   VROD_F32_SPLIT = 0 | 1   fp32 handles: never | always scan batches through the
 *                            bf16 [hi | lo] planes (default: while the planes fit)
 *   VROD_RCCL = 0            multi-device handles exchange their lists by peer copies
 *                            instead of the RCCL all-gather
 *   VROD_RCCL_LIB = path     the RCCL library to bind (nothing else is tried; a path
 *                            that does not load means peer copies, said once on stderr)
 */
#ifndef VROD_H
#define VROD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vrod_index vrod_index;

typedef enum {
    VROD_OK = 0,
    VROD_ERR_INVALID_ARG = 1,   /* null pointer, zero dim, bad enum, k too large ... */
    VROD_ERR_INVALID_VALUE = 2, /* NaN or Inf in rows or queries */
    VROD_ERR_NO_DEVICE = 3,     /* no usable gfx950 device / HIP runtime failure at open */
    VROD_ERR_OUT_OF_MEMORY = 4,
    VROD_ERR_HIP = 5,           /* a HIP call failed; vrod_last_error() has the text */
    VROD_ERR_UNSUPPORTED = 6,
    VROD_ERR_INTERNAL = 7,
    VROD_ERR_CAPACITY = 8,      /* vrod_range_search: the result does not fit the caller's buffers (out_lims is valid) */
    VROD_ERR_IO = 9,            /* snapshots: open / read / write / rename / fsync failed; vrod_last_error() carries errno's text */
    VROD_ERR_CORRUPT = 10       /* snapshots: not a snapshot, a truncated file, sizes that disagree, a checksum mismatch */
} vrod_status;

enum { VROD_DTYPE_F32 = 0, VROD_DTYPE_BF16 = 1 };  /* storage + fast-pass type */
enum { VROD_METRIC_COSINE = 0, VROD_METRIC_L2 = 1, VROD_METRIC_IP = 2 };

#define VROD_ID_NONE UINT64_MAX
#define VROD_MAX_K 3584u
#define VROD_MAX_DIM 32768u   /* one prepared row (fp32) must fit in a work-group's LDS next to its tiles */

/* Which fast pass vrod_search uses. AUTO picks by batch size and dtype. */
enum { VROD_PATH_AUTO = 0, VROD_PATH_STREAM = 1, VROD_PATH_MFMA = 2, VROD_PATH_EXACT = 3,
       VROD_PATH_GATHER = 4 };   /* filtered searches: canonical scores of the eligible rows only */

/* Counters of the most recently COMPLETED search on a handle (bench.py / tests read these). */
typedef struct {
    uint32_t path;              /* VROD_PATH_* actually taken */
    uint32_t nq, k, kprime;     /* kprime = candidates re-scored per query (k + a margin that follows the certificates:
                                 * doubled after a search in which some failed, halved after 64 clean searches) */
    uint32_t scan_launches;     /* launches of the dominant scan kernel */
    uint32_t fallback_queries;  /* queries whose certificate failed -> exact path */
    float scan_ms;              /* HIP-event time of the scan kernel launches (sum, sample pass included) */
    float total_ms;             /* HIP-event time of the whole device pipeline */
    double scan_bytes;          /* algorithmic corpus bytes the scan launches covered */
    double scan_flops;          /* algorithmic flops (2*Q*N*d) of the scan launches */
    float max_fast_err;         /* max |fast - canonical| over re-scored candidates (relative to
                                 * |canonical| on the direct-L2 stream path, whose bound is relative) */
    float eps_bound;            /* the certificate's bound on that error */
    uint32_t split_pass;        /* 1: the batched fast pass of an F32 handle ran on its bf16 [hi | lo] planes */
    uint32_t band_queries;      /* of the fallback_queries: resolved by the band pass (one more shared scan that
                                 * collects the rows within the error bound of the k-th score), not the exact path */
    float sample_ms;            /* of scan_ms: the sample-pass launch of a staged MFMA search (its own kernel form; it
                                 * sets the first thresholds and covers no algorithmic work -- its rows are scanned
                                 * again by the first filtered launch); 0 when the search had none */
    uint32_t exchange;          /* multi-device handle: how the per-shard lists reached the merge --
                                 * 0 none (single device), 1 RCCL all-gather, 2 peer copies (VROD_RCCL=0) */
    float overlap_ms;           /* of scan_ms: how long this search's sample-pass launch and the PREVIOUS search's last scan
                                 * launch were both in flight (pipelined searches over up to 6M rows put the two side by
                                 * side; each launch's own time then includes waiting for compute units).  The sum of
                                 * scan_ms - overlap_ms over a run = the time at least one scan launch was in flight */
} vrod_search_stats;

/* --- lifecycle ------------------------------------------------------------- */
/* device_ids/n_devices: the GPUs the corpus is sharded over.  n_devices <= 1: one
 * handle drives one GPU (bench.py's default deployment is one process and one handle per GPU, see
 * vrod_search_device + vrod_merge_topk_device).  n_devices > 1 (at most 64, an id may repeat): ONE
 * handle owns a shard on every listed device -- the single-process model of SURVEY.md 8e, all a
 * host like vRod (Rc<RefCell<Database>>, one thread) needs.  Rows are dealt to the shards in blocks
 * of 65536 in insertion order; a search runs on every shard at once; the per-shard top-k lists are
 * exchanged with ONE ncclAllGather per device (RCCL, communicator from ncclCommInitAll over the
 * distinct devices, one exchange stream per device, inside ncclGroupStart/End) and merged on
 * device_ids[0]; ids are global insertion indices as for a single device.  librccl is loaded when
 * the first such handle is created (VROD_RCCL_LIB: its path; VROD_RCCL=0: peer copies to the first
 * device instead of RCCL).  Device pointers passed to such a handle live on device_ids[0].  The
 * pipelined _begin_/_end form works as for one device: while the exchange and merge of batch s run,
 * every device already scans batch s+1. */
int vrod_index_create(vrod_index **out, uint32_t dim, int dtype, int metric,
                      const int *device_ids, int n_devices);
int vrod_index_destroy(vrod_index *idx);

/* --- corpus ---------------------------------------------------------------- */
int vrod_index_reserve(vrod_index *idx, uint64_t n_rows);
/* rows: n x dim fp32, row-major, host memory. Normalised (COSINE only) and converted
 * (BF16) on the device. Ids continue from the current count. */
int vrod_index_add(vrod_index *idx, const float *rows, uint64_t n);
/* Append rows [first_row, first_row+n) of the synthetic stream `seed`
 * (random unit vectors), generated on the device. */
int vrod_index_add_synthetic(vrod_index *idx, uint64_t seed, uint64_t first_row, uint64_t n);
int vrod_index_count(const vrod_index *idx, uint64_t *out_count);
/* Shard support: reported id = local row index + offset. */
int vrod_index_set_id_offset(vrod_index *idx, uint64_t offset);
/* Delete rows (<- vRod's DELETE, src/command/types.rs, builder.rs): `ids` (host memory, n of them) are ids as searches
 * report them, id_offset applied.  Afterwards no search on the handle -- any path, dtype or metric, pipelined,
 * replayed, multi-device, band or exact -- returns those rows: the results are bit for bit those of the same search
 * over the live rows alone (ties still broken by smaller id; slots beyond the live rows are (VROD_ID_NONE, NaN)).
 * Deleting a row again, or naming it twice in one call, is fine.  An id that is not a current row (below the offset,
 * or id - offset >= count) fails the whole call with VROD_ERR_INVALID_ARG and deletes nothing; n == 0 does nothing.
 * Ids are never reused until vrod_index_compact renumbers them: vrod_index_count still counts every row ever added
 * (and is the next id), vrod_index_get_rows still reads deleted rows back, and vrod_search_stats scan_bytes /
 * scan_flops still count every stored row. */
int vrod_index_delete(vrod_index *idx, const uint64_t *ids, uint64_t n);
/* Update rows in place (<- vRod's UPDATE, src/command/types.rs:82, builder.rs:53): row ids[i] (host memory, ids as
 * searches report them, id_offset applied) gets the vector rows[i] (n x dim fp32, host memory), prepared exactly as
 * vrod_index_add prepares it (normalised for COSINE, bf16-rounded on BF16 handles), and keeps its id.  Afterwards
 * every search -- any entry point, path, dtype or metric, pipelined, replayed, multi-device, range, band or exact,
 * with a filter and deletions in place -- and vrod_index_get_rows give bit for bit what they give on a fresh handle
 * built from the rows given to vrod_index_add with rows[i] put in place of row ids[i], in order: an id named twice
 * takes the last vector.  An id that is not a current row (below the offset, id - offset >= count, or a deleted row)
 * fails the whole call with VROD_ERR_INVALID_ARG, a NaN or Inf anywhere in `rows` with VROD_ERR_INVALID_VALUE; a
 * failed call changes nothing.  n == 0 does nothing.  Counts, deletions and the filter are unchanged.  The
 * certificate's bound (vrod_search_stats eps_bound) may stay wider than a fresh handle's -- it follows the largest
 * row norm the handle has ever held -- the results do not differ.  While a search is pending: VROD_ERR_INVALID_ARG. */
int vrod_index_update(vrod_index *idx, const uint64_t *ids, const float *rows, uint64_t n);
/* Compact (<- vRod's REINDEX, src/command/types.rs:134, builder.rs:73): physically remove every deleted row, in
 * place.  The surviving rows keep their order and are renumbered densely: the survivor with the j-th smallest id gets
 * id offset + j.  Afterwards the handle is indistinguishable from a fresh handle with the same id_offset to which
 * only the surviving rows were added, in order: vrod_index_count = vrod_index_live_count = the old live count,
 * vrod_index_get_rows, every search and range search (ids and score bits), and their scan_bytes / scan_flops --
 * deleted rows stop costing scan time.  A filter that is set follows its rows (vrod_index_filter_count is unchanged).
 * out_new_ids (host memory, may be NULL): map_len must equal vrod_index_count before the call (else
 * VROD_ERR_INVALID_ARG, nothing changes); entry i receives the new id of old id offset + i, or VROD_ID_NONE if that
 * row was deleted.  With nothing deleted nothing moves and the map is the identity.  The allocation is kept: the freed
 * rows serve later adds.  Multi-device handles: VROD_ERR_UNSUPPORTED, nothing changes.  While a search is pending:
 * VROD_ERR_INVALID_ARG.  Every check and allocation comes before the first row moves; a VROD_ERR_HIP after that
 * leaves the handle unusable (vrod_last_error says so): destroy it. */
int vrod_index_compact(vrod_index *idx, uint64_t *out_new_ids, uint64_t map_len);
/* Rows added minus rows deleted. */
int vrod_index_live_count(const vrod_index *idx, uint64_t *out);
/* Allow-list filter (one per handle): every search after this call -- any entry point, path, dtype or metric,
 * pipelined, replayed, multi-device -- returns bit for bit what the same search returns over the ELIGIBLE rows alone
 * (live and allowed; ties still broken by smaller id; slots beyond the eligible rows are (VROD_ID_NONE, NaN)), until
 * the filter is cleared or replaced.  allow_words: host memory, ceil(n_rows/32) words in the deleted-row layout: bit
 * i % 32 of word i / 32 set = id offset + i is allowed.  Rows at index >= n_rows are not allowed, rows added later
 * included.  n_rows > count: VROD_ERR_INVALID_ARG, nothing changes.  (NULL, 0) clears the filter.  Deletes made
 * after the call are honoured.  A multi-device handle routes the bits to its shards (global ids, as deletes).
 * While a search is pending: VROD_ERR_INVALID_ARG.  vrod_index_set_filter_where makes the bits from a predicate over the
 * rows' tags, values and labels on the device: the where-clause of the search forms that take no predicate. */
int vrod_index_set_filter(vrod_index *idx, const uint32_t *allow_words, uint64_t n_rows);
/* Rows the next search may return: live and allowed (= vrod_index_live_count without a filter). */
int vrod_index_filter_count(const vrod_index *idx, uint64_t *out);
/* Row labels: every row carries one uint32_t label -- 0 until set, and 0 for rows added later -- that only
 * vrod_search_labeled and vrod_search_grouped read (vrod_search, vrod_range_search and the pipelined forms ignore
 * labels entirely).  set_labels gives the rows with ids [first_id, first_id + n) (ids as searches report them, id_offset applied; deleted rows may be
 * named) the labels labels[0 .. n) (host memory); a range that is not wholly within the current rows fails with
 * VROD_ERR_INVALID_ARG and changes nothing; n == 0 does nothing.  vrod_index_update keeps a row's label,
 * vrod_index_delete leaves labels alone, vrod_index_compact moves them with their rows.  get_labels reads them back
 * (host memory).  Labels cost nothing until first set: the device array is allocated by the first set_labels.  While a
 * search is pending: VROD_ERR_INVALID_ARG.  Multi-device handles: set_labels returns VROD_ERR_UNSUPPORTED and changes
 * nothing (get_labels reports the zeros every row carries). */
int vrod_index_set_labels(vrod_index *idx, uint64_t first_id, const uint32_t *labels, uint64_t n);
int vrod_index_get_labels(vrod_index *idx, uint64_t first_id, uint64_t n, uint32_t *out_labels);
/* Row tags: every row carries one uint64_t tag mask -- 0 until set, and 0 for rows added later -- that only
 * vrod_search_tagged reads (every other search ignores tags entirely; tags and labels are independent).  set_tags gives
 * the rows with ids [first_id, first_id + n) (ids as searches report them, id_offset applied; deleted rows may be
 * named) the masks tags[0 .. n) (host memory); a range that is not wholly within the current rows fails with
 * VROD_ERR_INVALID_ARG and changes nothing; n == 0 does nothing.  vrod_index_update keeps a row's tags,
 * vrod_index_delete leaves tags alone, vrod_index_compact moves them with their rows.  get_tags reads them back (host
 * memory).  Tags cost nothing until first set: the device array is allocated by the first set_tags.  While a search is
 * pending: VROD_ERR_INVALID_ARG.  Multi-device handles: set_tags returns VROD_ERR_UNSUPPORTED and changes nothing
 * (get_tags reports the zeros every row carries). */
int vrod_index_set_tags(vrod_index *idx, uint64_t first_id, const uint64_t *tags, uint64_t n);
int vrod_index_get_tags(vrod_index *idx, uint64_t first_id, uint64_t n, uint64_t *out_tags);
/* Row values: every row carries one signed 64-bit value -- 0 until set, and 0 for rows added later -- that only
 * vrod_search_where reads (every other search ignores values entirely; values, tags and labels are independent): a
 * timestamp, a price, a version.  The rules are those of the tags: set_values gives the rows with ids [first_id,
 * first_id + n) (ids as searches report them, id_offset applied; deleted rows may be named) the values values[0 .. n)
 * (host memory); a range that is not wholly within the current rows fails with VROD_ERR_INVALID_ARG and changes nothing;
 * n == 0 does nothing.  vrod_index_update keeps a row's value, vrod_index_delete leaves values alone, vrod_index_compact
 * moves them with their rows.  get_values reads them back (host memory).  Values cost nothing until first set: the device
 * array is allocated by the first set_values.  While a search is pending: VROD_ERR_INVALID_ARG.  Multi-device handles:
 * set_values returns VROD_ERR_UNSUPPORTED and changes nothing (get_values reports the zeros every row carries). */
int vrod_index_set_values(vrod_index *idx, uint64_t first_id, const int64_t *values, uint64_t n);
int vrod_index_get_values(vrod_index *idx, uint64_t first_id, uint64_t n, int64_t *out_values);
/* Row keys: every row carries one uint64_t key chosen by the caller -- VROD_ID_NONE ("no key") until set, and for rows
 * added later -- that names the row across vrod_index_compact, which renumbers ids.  No search reads keys; ids stay
 * insertion indices and every other entry point returns what it returns on a handle without keys.
 * set_keys / get_keys follow the rules of the values: the rows with ids [first_id, first_id + n) (ids as searches report
 * them, id_offset applied; deleted rows may be named) take keys[0 .. n) (host memory); a range that is not wholly within
 * the current rows fails with VROD_ERR_INVALID_ARG and changes nothing; n == 0 does nothing; the device arrays are
 * allocated by the first set_keys; while a search is pending: VROD_ERR_INVALID_ARG; multi-device handles:
 * VROD_ERR_UNSUPPORTED (get_keys reports VROD_ID_NONE for every row).  And one rule of their own:
 *   uniqueness  after a successful call no two LIVE rows hold the same key; VROD_ID_NONE may repeat, and setting it clears
 *               a row's key.  A call in which two live rows of the range would get the same key, or which gives a live
 *               row a key that a live row outside the range holds, fails with VROD_ERR_INVALID_ARG and changes nothing.
 *               Re-keying is fine: a permutation of the range's keys, the same keys again; a row's old key is free once
 *               the call succeeds.  Keys given to deleted rows are stored and read back by get_keys, are never found and
 *               take no part in uniqueness.
 * vrod_index_update keeps a row's key, vrod_index_delete frees it (the key is no longer found and may be given to another
 * row), vrod_index_compact moves keys with their rows, a snapshot holds them once they were set (a file in which two live
 * rows share a key: VROD_ERR_CORRUPT at load; builds older than the section answer VROD_ERR_UNSUPPORTED to such a file).
 * The keys are found through an open-addressing table in device memory (linear probing, a power of two of slots, at
 * least 1024; DESIGN.md "Row keys").  The home slot of a key is part of this contract: z = key + 0x9E3779B97F4A7C15,
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^= z >> 31, home = z & (slots - 1),
 * all mod 2^64 (the mixer of the snapshot checksum).  Slots of deleted or re-keyed rows stay behind; the occupied slots,
 * those included, never exceed slots / 2: before an insert could cross that, the table is rebuilt from the live keyed
 * rows, doubled until they and the incoming keys fit in a quarter of it.  It is also rebuilt by vrod_index_compact and
 * built by vrod_index_load.  Every walk is bounded by the slot count: one that runs out is VROD_ERR_INTERNAL, not a hang.
 *   find_keys     out_ids[i] = the id (id_offset applied) of the live row that holds keys[i]; VROD_ID_NONE for a key no
 *                 live row holds and for VROD_ID_NONE itself.  Keys may repeat.  The filter is not consulted: a key names
 *                 a row whether or not the next search may return it.  Keys never set: every answer is VROD_ID_NONE.
 *   ids_to_keys   out_keys[i] = the key row ids[i] stores -- a deleted row's too -- or VROD_ID_NONE for VROD_ID_NONE (an
 *                 unfilled result slot), an id that is not a current row, or a row without a key: it turns any search's
 *                 nq x k ids into the caller's names.
 *   The _device forms take device pointers and a stream (the caller's work on it is complete before the library starts)
 *   and return after the results are complete in device memory.  All four: VROD_ERR_INVALID_ARG while a search is pending,
 *   VROD_ERR_UNSUPPORTED on multi-device handles, outputs untouched.
 *   delete_keys   deletes the live row of each key as vrod_index_delete would; a key no live row holds is ignored (lists
 *                 kept outside outlive deletes), repeats are fine; *out_deleted (may be NULL) = rows that died.
 *   upsert        rows: n x dim fp32, host memory.  If a live row holds keys[i] it is updated in place exactly as
 *                 vrod_index_update would (it keeps its id, label, tags and value); otherwise rows[i] is appended exactly
 *                 as vrod_index_add would and gets the key; appended rows take the next ids in the order of the call.
 *                 out_ids (may be NULL) receives each key's id.  VROD_ID_NONE as a key or a key twice in one call:
 *                 VROD_ERR_INVALID_ARG; NaN or Inf anywhere in rows: VROD_ERR_INVALID_VALUE; every check comes before
 *                 the first row is written, a refused call changes nothing.  Afterwards every search gives bit for bit
 *                 what it gives on a handle that had the same update and add calls made on it.
 * vrod_index_key_stats: all zero before the first set_keys. */
typedef struct {
    uint64_t keyed_live;   /* live rows with a key */
    uint64_t slots;
    uint64_t occupied;     /* slots in use, stale ones included */
    uint64_t rebuilds;     /* since the handle was created or loaded */
    uint64_t max_probe;    /* the longest walk an insert or rebuild has made since the last rebuild, in slots */
} vrod_key_stats;
int vrod_index_set_keys(vrod_index *idx, uint64_t first_id, const uint64_t *keys, uint64_t n);
int vrod_index_get_keys(vrod_index *idx, uint64_t first_id, uint64_t n, uint64_t *out_keys);
int vrod_index_find_keys(vrod_index *idx, const uint64_t *keys, uint64_t n, uint64_t *out_ids);
int vrod_index_find_keys_device(vrod_index *idx, const uint64_t *d_keys, uint64_t n, uint64_t *d_out_ids, void *stream);
int vrod_index_ids_to_keys(vrod_index *idx, const uint64_t *ids, uint64_t n, uint64_t *out_keys);
int vrod_index_ids_to_keys_device(vrod_index *idx, const uint64_t *d_ids, uint64_t n, uint64_t *d_out_keys, void *stream);
int vrod_index_delete_keys(vrod_index *idx, const uint64_t *keys, uint64_t n, uint64_t *out_deleted);
int vrod_index_upsert(vrod_index *idx, const uint64_t *keys, const float *rows, uint64_t n, uint64_t *out_ids);
int vrod_index_key_stats(const vrod_index *idx, vrod_key_stats *out);
/* Copy prepared rows [first, first+n) back as fp32 (bf16 widened): n x dim. */
int vrod_index_get_rows(vrod_index *idx, uint64_t first, uint64_t n, float *out_rows);

/* --- device-resident ingest ------------------------------------------------ */
/* add / update / upsert / get_rows for callers whose rows are in GPU memory already (an encoder's output, often fp16 or
 * bf16 and a slice of a larger buffer): the row payload never crosses to the host.
 *   source      d_rows is device memory holding n rows of src_dtype elements: row i starts at element i * row_stride and
 *               dim consecutive elements follow.  row_stride is in elements and must be >= dim (there is no "0 means
 *               dim"); the pointer need only be aligned to its element (4 bytes for F32, 2 for BF16 / F16): the library
 *               uses wide loads only where the address allows them.  n * row_stride overflowing 64 bits, a misaligned
 *               pointer, a null idx, a null d_rows (d_ids, d_keys) with n > 0, an unknown src_dtype:
 *               VROD_ERR_INVALID_ARG, checked before any device call.  The padding between rows is never read.
 *   conversion  BF16 and F16 elements are widened to fp32 exactly (fp16 subnormals included, -0.0 kept); from there every
 *               row is treated exactly as vrod_index_add / _update / _upsert treat the same fp32 values: the fp64
 *               left-to-right norm chain and (f32)((f64)x / nrm) under COSINE, the bf16 rounding of a BF16 handle after
 *               it (a bf16 source on a bf16 cosine handle is still normalised and rounded again).
 *   result      after any sequence of these calls the handle is indistinguishable through this ABI from one on which the
 *               host forms were called with the widened rows: get_rows, every search (ids and score bits), eps_bound,
 *               scan_bytes, count / live_count and the bytes vrod_index_save writes.
 *   bad values  NaN or Inf anywhere in the n x dim elements read (for F16: the encodings 0x7C00.. and 0xFC00..):
 *               VROD_ERR_INVALID_VALUE; a refused call changes nothing (rows, norms, the certificate's bound, count, key
 *               table), and every check comes before the first row of an update or upsert is written.
 *   ids, keys   d_ids / d_keys / d_out_ids (may be NULL) are device memory; validation and semantics are those of the host
 *               forms (an id that is not a current row or names a deleted row fails the call, an id twice takes the last
 *               vector, VROD_ID_NONE as a key or a key twice fails the call, appended rows take the next ids in call
 *               order).  These 8 bytes per row are copied to the host for the checks; the rows are not.
 *   stream      as vrod_index_find_keys_device: the caller's work on `stream` (may be NULL) is complete before the library
 *               reads, and the call returns when the rows are in place.
 *   state       while a search is pending: VROD_ERR_INVALID_ARG.
 *   get_rows_device  vrod_index_get_rows into device memory: n rows of dim fp32, row i at element i * out_row_stride
 *               (>= dim) of d_out_rows; the padding between the rows is not written.
 *   multi-device handles  add_device, update_device and get_rows_device deal rows and ids to the shards as the host forms
 *               do (every shard checks its rows of an update before any shard writes one); a source on another device
 *               than a shard is packed there, copied peer to peer in the host forms' chunks and ingested from the copy.
 *               upsert_device: VROD_ERR_UNSUPPORTED, as vrod_index_upsert. */
typedef enum { VROD_SRC_F32 = 0, VROD_SRC_BF16 = 1, VROD_SRC_F16 = 2 } vrod_src_dtype;
int vrod_index_add_device(vrod_index *idx, const void *d_rows, int src_dtype, uint64_t row_stride, uint64_t n, void *stream);
int vrod_index_update_device(vrod_index *idx, const uint64_t *d_ids, const void *d_rows, int src_dtype, uint64_t row_stride,
                             uint64_t n, void *stream);
int vrod_index_upsert_device(vrod_index *idx, const uint64_t *d_keys, const void *d_rows, int src_dtype, uint64_t row_stride,
                             uint64_t n, uint64_t *d_out_ids, void *stream);
int vrod_index_get_rows_device(vrod_index *idx, uint64_t first, uint64_t n, float *d_out_rows, uint64_t out_row_stride,
                               void *stream);

/* --- snapshots ------------------------------------------------------------- */
/* A snapshot is one file that holds the whole observable state of a single-device handle; a handle loaded from it is
 * indistinguishable from the one that was saved, to the bit (<- the reference's Database::load, src/database/mod.rs,
 * which is todo!()).  The format (version 1, little-endian; DESIGN.md "Snapshots") is a 4096-byte header -- magic
 * "VRODSNAP", version, the scalars of vrod_snapshot_info, a table of sections (kind, offset, payload bytes, checksum) and
 * its own checksum -- and the sections, each on a 4096-byte boundary, zero-padded; all offsets and lengths are 64-bit.
 *   saved       dim, dtype, metric, count, id_offset; the prepared rows as stored (bf16 or fp32, never rounded again),
 *               DENSE: [count][dim] elements, the row pitch is not part of the format; the per-row squared norms; the
 *               largest squared norm the handle has ever held (it keeps vrod_search_stats eps_bound the same); the
 *               deleted-row bits; the allowed bits of a filter, if one is set; labels, tags and values, each only if it
 *               was ever set -- "never set" survives the round trip, those arrays still cost nothing until first set.
 *   not saved   vrod_index_set_path, the profiling level, the last stats (vrod_index_last_stats, _last_multivec), the
 *               bf16 [hi | lo] planes of an F32 handle (rebuilt at the next batched search), the self-tuned candidate
 *               margin (kprime starts over) and spare capacity (vrod_index_reserve).
 * vrod_index_save writes to "<path>.tmp", fsyncs and renames it over `path`: a failure of any kind removes the temporary
 * file and leaves an older file at `path` as it was.  The handle is left exactly as it was found: every search after the
 * call gives what it gave before it, captured graphs included.  The bytes depend on the state alone (no timestamps, zero
 * padding): saving twice gives identical files, and so does save, load, save.  Null arguments, or a search pending:
 * VROD_ERR_INVALID_ARG; a multi-device handle: VROD_ERR_UNSUPPORTED, nothing is written; the file system refusing:
 * VROD_ERR_IO.
 * vrod_index_load creates a handle (as vrod_index_create does: VROD_F32_SPLIT applies, n_devices <= 1, device_ids[0] or
 * device 0) that matches the saved one in every observable of this header: vrod_index_count, _live_count, _filter_count,
 * _get_rows, _get_labels, _get_tags, _get_values, every search entry point (ids and score bits, a NaN matching any NaN),
 * eps_bound, scan_bytes and scan_flops; later mutations behave as they would have on the original.  Everything that can
 * be checked without a device is checked before the first device call -- the header, the version, the section table
 * against the file's real length, and the checksum of every section of at most 1 MiB -- so a bad file fails the same way
 * on a machine without a GPU.  Every section's checksum is verified: the rows and the larger arrays by the device, over
 * the bytes as they arrived in its memory (the host never makes a pass over them).  Not a snapshot, truncated, sizes that
 * disagree, a checksum mismatch: VROD_ERR_CORRUPT; another version, or section kinds this build does not know:
 * VROD_ERR_UNSUPPORTED; n_devices > 1: VROD_ERR_UNSUPPORTED; open or read failing: VROD_ERR_IO.  On any failure *out is
 * NULL and nothing is kept.  A snapshot loads onto the dtype and metric it was saved with, nothing else.
 * Rows move between the device and the file in chunks (a multiple of 32 rows, 32 MiB by default) through two pinned host
 * buffers on the handle's stream: the pack / unpack kernel and the copy of one chunk run beside the file I/O of its
 * neighbour.  VROD_DEBUG_SNAPSHOT_CHUNK_ROWS (read at every call) sets the rows per chunk.
 * vrod_snapshot_info reads the header alone; vrod_snapshot_verify checks the whole file on the host.  Neither needs a device.
 * The section checksum: with w_i the payload's little-endian u32 words (the last one zero-filled) and i = first_word +
 * the word's position, z = w_i + (i + 1) * 0x9E3779B97F4A7C15, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9,
 * z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^= z >> 31, all mod 2^64; the checksum is the sum of the z mod 2^64, so any
 * chunking or order gives the same value.  vrod_snapshot_checksum computes it on the host, _checksum_device over device
 * memory (d_bytes 4-byte aligned; `out` is host memory, written when the call returns). */
struct vrod_snapshot_info {   /* (a struct tag, not a typedef: the function below has the same name, as stat(2) does) */
    uint32_t version, dim, dtype, metric;
    uint64_t count, live_count, id_offset, file_bytes;
    uint32_t has_filter, has_labels, has_tags, has_values;
};
int vrod_index_save(vrod_index *idx, const char *path);
int vrod_index_load(vrod_index **out, const char *path, const int *device_ids, int n_devices);
int vrod_snapshot_info(const char *path, struct vrod_snapshot_info *out);
int vrod_snapshot_verify(const char *path);
int vrod_snapshot_checksum(const void *bytes, uint64_t n_bytes, uint64_t first_word, uint64_t *out);
int vrod_snapshot_checksum_device(int device, const void *d_bytes, uint64_t n_bytes, uint64_t first_word,
                                  uint64_t *out, void *stream);

/* --- search ---------------------------------------------------------------- */
/* queries: nq x dim fp32 host; out_ids: nq x k; out_scores: nq x k. */
int vrod_search(vrod_index *idx, const float *queries, uint32_t nq, uint32_t k,
                uint64_t *out_ids, float *out_scores);
/* Same with device pointers (queries, outputs) and a HIP stream (hipStream_t, may be
 * NULL). Returns after the results are complete in device memory. */
int vrod_search_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k,
                       uint64_t *d_out_ids, float *d_out_scores, void *stream);
/* Queries from the synthetic stream, generated on the device (bench / tests). */
int vrod_search_synthetic_device(vrod_index *idx, uint64_t seed, uint64_t first_row,
                                 uint32_t nq, uint32_t k, uint64_t *d_out_ids,
                                 float *d_out_scores, void *stream);
/* Pipelined form of vrod_search_device: _begin_ enqueues the whole search on the library's own
 * stream, ordered after everything `stream` holds at the time of the call, and returns without
 * waiting for the device; vrod_search_end completes the OLDEST begun search (FIFO) -- when it
 * returns VROD_OK that search's results are complete in device memory.  At most two searches may
 * be pending: begin(s+1) before end(s) keeps the device busy while the host, and the caller's
 * exchange of batch s (all-gather + merge), catch up.  A begun search must be
 * ended; the queries of a _begin_device call and both output buffers must stay untouched until
 * then.  While a search is pending every other entry point on the handle that touches the
 * corpus or the stream fails with VROD_ERR_INVALID_ARG.  Errors that depend on the data (NaN or
 * Inf in the queries) are reported by vrod_search_end. */
int vrod_search_begin_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k,
                             uint64_t *d_out_ids, float *d_out_scores, void *stream);
int vrod_search_begin_synthetic_device(vrod_index *idx, uint64_t seed, uint64_t first_row,
                                       uint32_t nq, uint32_t k, uint64_t *d_out_ids,
                                       float *d_out_scores, void *stream);
int vrod_search_end(vrod_index *idx);
int vrod_search_pending(const vrod_index *idx, uint32_t *out_pending);

/* Range search: EVERY eligible row (live, and allowed while a filter is set) whose canonical score s is at least as
 * good as the query's threshold -- s >= thresholds[q] (COSINE, IP), s <= thresholds[q] (L2), compared as fp32 values:
 * the boundary is inclusive, -0.0 == +0.0, a NaN score never qualifies.  Exact, like a search: ids and score bits are
 * the CPU oracle's.  There is no k and VROD_MAX_K does not apply: one query may return every row.
 *   thresholds  nq floats in the units of the handle's scores; NaN -> VROD_ERR_INVALID_VALUE, +-inf allowed.
 *               Queries are prepared exactly as vrod_search prepares them.
 *   out_lims    nq + 1 entries: out_lims[0] = 0, out_lims[q + 1] - out_lims[q] = qualifying rows of query q.  Always
 *               exact and always written once the call gets as far as scanning, whatever `capacity` is.
 *   capacity    entries out_ids / out_scores hold.  out_lims[nq] <= capacity: VROD_OK, entries [out_lims[q],
 *               out_lims[q + 1]) are query q's rows, best first, ties by smaller id (id_offset applied); entries past
 *               out_lims[nq] are not touched.  out_lims[nq] > capacity: VROD_ERR_CAPACITY, out_ids / out_scores are
 *               unspecified, out_lims is valid -- a second call with capacity >= out_lims[nq] succeeds.  capacity = 0
 *               with null out_ids / out_scores is the count-only form.
 * nq = 0: VROD_OK with out_lims[0] = 0; an empty handle: all-zero out_lims.  Fails with VROD_ERR_INVALID_ARG while a
 * search is pending; there is no pipelined form and no graph replay (the output size depends on the data).
 * vrod_index_set_path is honoured (EXACT: canonical scores of every row; GATHER: of the eligible rows; STREAM has no
 * threshold form and is treated as AUTO).  vrod_index_last_stats afterwards: path = the route taken, k = 0, kprime =
 * the largest per-query candidate count of the fast pass, fallback_queries = queries answered by the canonical route.
 * The _device form takes device pointers on the handle's first device and returns after the results are complete. */
int vrod_range_search(vrod_index *idx, const float *queries, uint32_t nq, const float *thresholds,
                      uint64_t capacity, uint64_t *out_lims, uint64_t *out_ids, float *out_scores);
int vrod_range_search_device(vrod_index *idx, const float *d_queries, uint32_t nq, const float *d_thresholds,
                             uint64_t capacity, uint64_t *d_out_lims, uint64_t *d_out_ids, float *d_out_scores,
                             void *stream);

/* Labelled search -- one batch, a label per query (mixed-tenant batches): query q sees the rows that are live, allowed
 * by the handle's filter if one is set, and labelled query_labels[q] (nq words, host memory; the _device form: device
 * memory).  Its result row is bit for bit (ids and score bits, a NaN matching any NaN) what vrod_search returns for that
 * query on a fresh handle that holds only those rows, in order, with the ids mapped back: ties break by smaller id, slots
 * beyond the matching rows are (VROD_ID_NONE, NaN), a label no row carries gives a row of those.  A handle whose labels
 * were never set holds label 0 in every row.  k, null pointers and NaN / Inf in the queries are handled as vrod_search
 * handles them.  Synchronous, like a range search: no _begin_ form, no graph replay; VROD_ERR_INVALID_ARG while a search
 * is pending; the _device form returns after the results are complete in device memory.  The rows are grouped by the
 * batch's labels on the device, in one pass over the label array; a label with few rows has the canonical scores of its
 * own rows computed (all such labels of the batch in one launch), a label with a large share of the rows takes the
 * ordinary scan with the other labels masked (vrod_index_set_path: GATHER sends every label the first way, STREAM /
 * MFMA / EXACT the second).  vrod_index_last_stats afterwards: path = VROD_PATH_GATHER if no label took a scan, else the
 * path of the last scan; kprime, max_fast_err, eps_bound = maxima over the scans (0 without one); scan_launches,
 * fallback_queries, band_queries = sums; scan_bytes / scan_flops = the rows (x the queries) of each label scored on its
 * own, plus every stored row per scan.  Multi-device handles: VROD_ERR_UNSUPPORTED. */
int vrod_search_labeled(vrod_index *idx, const float *queries, uint32_t nq, uint32_t k,
                        const uint32_t *query_labels, uint64_t *out_ids, float *out_scores);
int vrod_search_labeled_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k,
                               const uint32_t *d_query_labels, uint64_t *d_out_ids, float *d_out_scores,
                               void *stream);

/* Tagged search -- one batch, a predicate over the row tags per query (attributes, access groups).  A row with tags t
 * matches the predicate p iff
 *     (p.any == 0 || (t & p.any) != 0)  &&  (t & p.all) == p.all  &&  (t & p.none) == 0,
 * and query q sees the rows that are live, allowed by the handle's filter if one is set, and matching preds[q] (nq
 * structs, host memory; the _device form: device memory, copied to the host to be grouped).  Labels are ignored.  Its
 * result row is bit for bit (ids and score bits, a NaN matching any NaN) what vrod_search returns for that query on a
 * fresh handle that holds only those rows, in order, with the ids mapped back: ties break by smaller id, slots beyond the
 * matching rows are (VROD_ID_NONE, NaN).  A predicate with all & none != 0 can match nothing: an all-unfilled row, without
 * a pass over the corpus.  {0, 0, 0} matches every row: the bits of vrod_search under the same filter and deletions.  A
 * handle whose tags were never set holds 0 in every row.  k, null pointers and NaN / Inf in the queries are handled as
 * vrod_search handles them; an empty handle gives all-unfilled rows without looking at the queries.  Synchronous, like
 * the labelled search: no _begin_ form, no graph replay; VROD_ERR_INVALID_ARG while a search is pending; the _device form
 * returns after the results are complete in device memory.  Queries with identical predicates form one group; every
 * group's matching rows are counted on the device in one pass over the tag array per 2048 distinct predicates; a
 * predicate with few rows has the canonical scores of its own rows computed (all such predicates of a pass in one
 * launch; a row is scored once for every such predicate it matches), a predicate with a large share of the rows takes
 * the ordinary scan with the other rows masked -- one scan per distinct wide predicate (vrod_index_set_path: GATHER
 * sends every predicate the first way, STREAM / MFMA / EXACT the second).  vrod_index_last_stats afterwards: as after
 * vrod_search_labeled, with "predicate" for "label".  Multi-device handles: VROD_ERR_UNSUPPORTED, outputs untouched. */
typedef struct {
    uint64_t any, all, none;
} vrod_tag_pred; /* 24 bytes, no padding */
int vrod_search_tagged(vrod_index *idx, const float *queries, uint32_t nq, uint32_t k,
                       const vrod_tag_pred *preds, uint64_t *out_ids, float *out_scores);
int vrod_search_tagged_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k,
                              const vrod_tag_pred *d_preds, uint64_t *d_out_ids, float *d_out_scores,
                              void *stream);

/* Search with a tags + value-interval predicate per query ("only rows newer than t", "price between a and b", usually
 * joined with a tenant or access group).  A row with tags t and value v matches the predicate p iff
 *     (p.any == 0 || (t & p.any) != 0)  &&  (t & p.all) == p.all  &&  (t & p.none) == 0  &&  p.lo <= v  &&  v <= p.hi,
 * the interval compared as signed values, both ends inclusive.  lo > hi, or all & none != 0, can match nothing: an
 * all-unfilled row, without a pass over the corpus.  {0, 0, 0, INT64_MIN, INT64_MAX} matches every row: the bits of
 * vrod_search under the same filter and deletions.  A handle whose tags (values) were never set holds 0 in every row.
 * Everything else is the contract of vrod_search_tagged: query q sees the live, allowed, matching rows and gets, bit for
 * bit, the top k over those rows in ascending id order (ties by smaller id, NaN last, unfilled slots (VROD_ID_NONE,
 * NaN)); k, null pointers, NaN / Inf in the queries, an empty handle and a pending search are handled the same way;
 * synchronous, no _begin_ form, no graph replay; vrod_index_set_path is honoured (GATHER: every predicate scored on its
 * own rows; STREAM / MFMA / EXACT: every predicate by a masked scan); vrod_index_last_stats reads as after a tagged
 * search; the _device form copies the predicates to the host to group them.  One pass over the tag and value arrays
 * serves 1024 distinct predicates.  Multi-device handles: VROD_ERR_UNSUPPORTED, outputs untouched. */
typedef struct {
    uint64_t any, all, none;
    int64_t lo, hi;
} vrod_where; /* 40 bytes, no padding */
int vrod_search_where(vrod_index *idx, const float *queries, uint32_t nq, uint32_t k,
                      const vrod_where *preds, uint64_t *out_ids, float *out_scores);
int vrod_search_where_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k,
                             const vrod_where *d_preds, uint64_t *d_out_ids, float *d_out_scores,
                             void *stream);

/* Row predicates -- the predicate of vrod_search_where, with the row's label beside it, as an operation on the rows
 * themselves: count them, list them, delete them, make them the filter, retag them.  A row with tags t, value v and
 * label l matches the predicate p iff
 *     (p.any == 0 || (t & p.any) != 0)  &&  (t & p.all) == p.all  &&  (t & p.none) == 0  &&  p.lo <= v  &&  v <= p.hi
 *     &&  (p.has_label == 0 || l == p.label),
 * the interval compared as signed values, both ends inclusive.  has_label is 0 or 1 (anything else:
 * VROD_ERR_INVALID_ARG); label is read only when it is 1.  A column that was never set holds 0 in every row.  lo > hi, or
 * all & none != 0, can match nothing and costs no pass over the corpus; {0, 0, 0, INT64_MIN, INT64_MAX, 0, 0} matches
 * every row.
 * Scope: every operation looks at the LIVE rows below vrod_index_count; with flags = VROD_ROWPRED_ALLOWED only at the
 * live rows the handle's filter allows -- the rows a search may return (without a filter the flag changes nothing).
 * Unknown flag bits: VROD_ERR_INVALID_ARG.  Rows between the count and the capacity (vrod_index_reserve) never match.
 * Common rules: single-device handles only -- a multi-device handle answers VROD_ERR_UNSUPPORTED, outputs and state
 * untouched; while a search is pending: VROD_ERR_INVALID_ARG; null required pointers: VROD_ERR_INVALID_ARG.  Every check
 * comes before the first write: a refused or failed call changes nothing.  vrod_index_last_stats is not touched.  Ids are
 * ids as searches report them, id_offset applied.  The three columns are read on the device and never cross to the host:
 * the host mirrors of a delete, a filter or a retag are updated from one bit per row.
 *   count_where   out_counts[i] = rows in scope matching preds[i] (n_preds structs and words, host memory).  Any
 *                 n_preds, repeats included; n_preds == 0 is VROD_OK; an empty handle gives zeros.  One pass over the
 *                 columns serves 1024 distinct predicates.
 *   select_where  the matching ids in ASCENDING order, under the capacity contract of vrod_range_search: *out_count (host
 *                 memory in both forms) is always exact; *out_count <= capacity: VROD_OK, out_ids[0 .. *out_count) filled,
 *                 entries past the count not touched; *out_count > capacity: VROD_ERR_CAPACITY, out_ids unspecified;
 *                 capacity == 0 with a null out_ids is the count-only form.  The _device form writes the ids to device
 *                 memory (they can feed vrod_search_candidates_device, vrod_index_update_device and
 *                 vrod_index_ids_to_keys_device without a host trip): the caller's work on `stream` is complete before
 *                 the library reads, as for vrod_index_find_keys_device, and the call returns when the ids are in place.
 *   delete_where  exactly what vrod_index_delete does with select_where's ids: tombstones, vrod_index_live_count and
 *                 vrod_index_filter_count drop, the dead rows' keys are free, and every search afterwards gives what it
 *                 gives after that vrod_index_delete.  *out_deleted (may be NULL) = rows that died.
 *   set_filter_where  exactly what vrod_index_set_filter(allow_words, n_rows = count) does with these bits: bit i set
 *                 iff row i is below the count and matches, WHETHER OR NOT IT IS DELETED; with VROD_ROWPRED_ALLOWED the
 *                 bit is also ANDed with the current filter's bit for the row, which narrows a filter instead of
 *                 replacing it.  Rows added later are not allowed; vrod_index_set_filter(NULL, 0) still clears; a
 *                 predicate that can match nothing gives a filter that allows nothing, not an error.  This is the
 *                 where-clause of every search form that honours the filter and takes no predicate of its own:
 *                 vrod_search and its pipelined forms, vrod_range_search, vrod_search_grouped, vrod_search_multivec,
 *                 vrod_search_diverse, vrod_search_by_ids, vrod_knn_graph, vrod_search_combined and the candidate
 *                 searches -- one predicate per call.
 *   set_tags_where  every matching row in scope gets t' = (t & ~clear_bits) | set_bits; set_bits & clear_bits != 0:
 *                 VROD_ERR_INVALID_ARG.  *out_changed (may be NULL) = rows whose mask actually changed.  On a handle
 *                 whose tags were never set, set_bits == 0 changes nothing and allocates nothing; otherwise this call
 *                 creates the column as the first vrod_index_set_tags would.  vrod_index_get_tags and a snapshot see the
 *                 new masks. */
#define VROD_ROWPRED_ALLOWED 1u
typedef struct {
    uint64_t any, all, none;   /* as vrod_tag_pred */
    int64_t lo, hi;            /* as vrod_where: signed, both ends inclusive */
    uint32_t label;            /* compared only when has_label == 1 */
    uint32_t has_label;        /* 0 or 1 */
} vrod_row_pred; /* 48 bytes, no padding */
int vrod_index_count_where(vrod_index *idx, const vrod_row_pred *preds, uint32_t n_preds, uint32_t flags,
                           uint64_t *out_counts);
int vrod_index_select_where(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags, uint64_t capacity,
                            uint64_t *out_count, uint64_t *out_ids);
int vrod_index_select_where_device(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags, uint64_t capacity,
                                   uint64_t *out_count, uint64_t *d_out_ids, void *stream);
int vrod_index_delete_where(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags, uint64_t *out_deleted);
int vrod_index_set_filter_where(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags);
int vrod_index_set_tags_where(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags, uint64_t set_bits,
                              uint64_t clear_bits, uint64_t *out_changed);

/* Ordered selection -- the first `limit` rows by their value, under a row predicate and after a keyset cursor: "the 100
 * newest rows of tenant L", "the next page", "the 1000 oldest rows to expire", without moving a column to the host.
 * Exact and deterministic; one device pass per call, nothing is persisted.
 * Rows considered: exactly the rows vrod_index_select_where(pred, flags & VROD_ROWPRED_ALLOWED) lists -- the live rows
 * below the count, under VROD_ROWPRED_ALLOWED only those the filter allows, that match pred.  The predicate rules are
 * those of the row-predicate block above: has_label is 0 or 1, a predicate that can match nothing costs no pass, a
 * column that was never set reads 0 in every row.
 * Order: by (value, id) ascending, the value compared as signed; with VROD_ORDER_DESC by value DESCENDING and, among
 * equal values, id STILL ASCENDING -- the smaller id wins ties everywhere in this library.  Ids are ids as searches
 * report them, id_offset applied; they are unique, so the order is total and no result depends on scheduling.
 * Cursor: after == NULL starts from the beginning.  Otherwise only rows STRICTLY after (after->value, after->id) in the
 * call's order are considered: ascending, v > value || (v == value && id > after->id); descending,
 * v < value || (v == value && id > after->id).  The cursor need not name a row that exists, is live or matches: a
 * deleted row, an id below id_offset, an id at or beyond the count and UINT64_MAX are all fine, which keeps pages
 * stable while rows are deleted, added and compacted between them.  The caller passes the last (value, id) of one
 * page as the cursor of the next.
 * Outputs: *out_total (may be NULL) = the considered rows after the cursor, exact: *out_total > *out_count says there
 * is more.  *out_count (required) = min(limit, total).  out_ids[0 .. *out_count) holds the ids in order, out_values
 * (may be NULL) their values; entries past the count are not touched.  limit == 0 is the count-only form: both arrays
 * may be NULL, the call is VROD_OK and *out_total is still exact.  limit > VROD_MAX_ORDERED: VROD_ERR_INVALID_ARG, as
 * k > VROD_MAX_K in vrod_search; longer listings page with the cursor.  There is no VROD_ERR_CAPACITY: limit is the
 * capacity.  In the _device form the two arrays are device memory on the handle's device and the two counts host
 * memory; the stream rule is vrod_index_select_where_device's: the caller's work on `stream` is complete before the
 * library reads, and the call returns with the arrays in place (they can feed vrod_search_candidates_device,
 * vrod_index_update_device and vrod_index_ids_to_keys_device without a host trip).
 * Common rules, as for the row predicates: unknown flag bits (anything outside 1u | 2u), a null pred or out_count, a
 * null out_ids with limit > 0: VROD_ERR_INVALID_ARG; while a search is pending: VROD_ERR_INVALID_ARG; a multi-device
 * handle: VROD_ERR_UNSUPPORTED.  Every check comes before the first write: a refused call writes nothing.
 * vrod_index_last_stats is not touched.  An empty handle gives zeros. */
#define VROD_ORDER_DESC   2u        /* shares the flags word with VROD_ROWPRED_ALLOWED (1u) */
#define VROD_MAX_ORDERED  65536u    /* rows one call returns; longer listings page with the cursor */
typedef struct {
    int64_t value;
    uint64_t id;
} vrod_order_cursor; /* 16 bytes, no padding */
int vrod_index_select_ordered(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags,
                              const vrod_order_cursor *after, uint32_t limit, uint64_t *out_count,
                              uint64_t *out_total, uint64_t *out_ids, int64_t *out_values);
int vrod_index_select_ordered_device(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags,
                                     const vrod_order_cursor *after, uint32_t limit, uint64_t *out_count,
                                     uint64_t *out_total, uint64_t *d_out_ids, int64_t *d_out_values,
                                     void *stream);

/* Row aggregation -- the GROUP BY of the row predicates: the rows a predicate matches, grouped by label, by value
 * bucket or by tag bit, with each group's row count, the min, max and sum of its values and its smallest id: "how many
 * chunks does each tenant hold", "rows per day about to expire", "rows per access group", "the oldest and newest row of
 * every document", without moving a column to the host.  Exact and deterministic; nothing is persisted.
 * Rows considered: exactly the rows vrod_index_select_where(pred, flags & VROD_ROWPRED_ALLOWED) lists, under the
 * predicate rules of the row-predicate block above: has_label is 0 or 1, a column that was never set reads 0 in every
 * row, a predicate that can match nothing costs no pass and gives zero groups.
 * Key (`by`):
 *   VROD_AGG_BY_LABEL  the row's label, 0 .. 2^32-1.  A handle that never set labels is one group with key 0.
 *   VROD_AGG_BY_VALUE  floor(value / width): FLOOR division on signed values (-1 / 10 gives -1), width >= 1 (anything
 *                      else: VROD_ERR_INVALID_ARG; width is read in this mode only).  Every result fits; with width 1
 *                      every int64 is a possible key, INT64_MIN, -1, 0 and INT64_MAX included.
 *   VROD_AGG_BY_TAG    a bit index 0 .. 63: a row counts -- with its value and its id -- in the group of EVERY tag bit it
 *                      has set, so there are at most 64 groups and the counts sum to the popcounts.  A row with tags 0
 *                      is in no group but is counted in *out_rows.
 * Aggregates per group: count; min_value and max_value compared as signed; sum_value the two's-complement sum, wrapping
 * mod 2^64; first_id the smallest id of the group, id_offset applied.  All five are commutative integer operations: no
 * result depends on scheduling, and repeated calls give identical bytes.
 * Outputs: *out_rows (may be NULL) = the rows considered, equal to vrod_index_count_where of the same predicate in all
 * three modes.  *out_groups (may be NULL) = the exact number of distinct groups.  *out_count (required) =
 * min(limit, groups).  out[0 .. *out_count) holds the first groups in the call's order; entries past the count are not
 * touched.  limit == 0 is the count-only form: out may be NULL.
 * Order: key ascending, compared as signed; with VROD_AGG_ORDER_COUNT count descending, then key ascending.  Keys are
 * unique within a result, so both orders are total.
 * More than VROD_MAX_AGG_GROUPS distinct groups: VROD_ERR_CAPACITY, and no output is written.
 * Common rules, as for the row predicates: unknown flag bits (anything outside 1u | 4u; 2u is VROD_ORDER_DESC's and
 * is refused here), by > 2, a null pred or out_count, a null out with limit > 0: VROD_ERR_INVALID_ARG; while a search
 * is pending: VROD_ERR_INVALID_ARG; a multi-device handle: VROD_ERR_UNSUPPORTED.  Every check comes before the first
 * write: a refused call writes nothing.  vrod_index_last_stats is not touched, the handle's state does not change, an
 * empty handle gives zeros.  The columns are read on the device and never cross to the host: only the groups do, which
 * the host then orders. */
#define VROD_AGG_BY_LABEL 0u       /* key = the row's label (0 .. 2^32-1) */
#define VROD_AGG_BY_VALUE 1u       /* key = floor(value / width), floor division on signed values, width >= 1 */
#define VROD_AGG_BY_TAG   2u       /* key = bit index 0..63; a row counts in the group of EVERY tag bit it has set */
#define VROD_AGG_ORDER_COUNT 4u    /* flags word shared with VROD_ROWPRED_ALLOWED (1u); 2u stays VROD_ORDER_DESC's and is refused here */
#define VROD_MAX_AGG_GROUPS 1048576u
typedef struct {
    int64_t  key;
    uint64_t count;       /* rows of the group */
    int64_t  min_value, max_value;
    int64_t  sum_value;   /* two's-complement sum, wrapping mod 2^64 */
    uint64_t first_id;    /* smallest id of the group, id_offset applied */
} vrod_agg_group; /* 48 bytes, no padding */
int vrod_index_aggregate_where(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags, uint32_t by, int64_t width,
                               uint32_t limit, uint64_t *out_count, uint64_t *out_groups, uint64_t *out_rows,
                               vrod_agg_group *out);

/* Group centroids -- the aggregate of the one column vrod_index_aggregate_where cannot take, the vectors: the mean (or
 * the sum) of the rows of every group, exact and independent of any order: "the embedding of a document as the mean of
 * its chunks", the centroid of a tenant or of a day's rows, a document-level index built from a chunk-level one.
 * Rows considered: exactly the rows vrod_index_select_where(pred, flags & VROD_ROWPRED_ALLOWED) lists, under the rules of
 * the row-predicate block above; deleted rows never, the filter only under the flag.
 * Key (`by`): VROD_AGG_BY_LABEL or VROD_AGG_BY_VALUE with the keys of vrod_index_aggregate_where, floor division
 * included; width is read under BY_VALUE only and must be >= 1.  VROD_AGG_BY_TAG and anything larger:
 * VROD_ERR_INVALID_ARG.
 * Outputs: the groups in ascending signed key order.  out_groups[g] = the key, the count and first_id (id_offset applied)
 * exactly as vrod_index_aggregate_where reports them for the same arguments.  Group g's dim floats start at
 * out_vectors + g * out_row_stride, out_row_stride >= dim; the floats between dim and the stride are not touched.
 * *out_count (required) = the number of groups, *out_rows (may be NULL) = the rows considered.
 * The value.  x: an element as vrod_index_get_rows reads it (the prepared row widened to fp32).  n: the handle's rows,
 * deleted ones included; R: the smallest integer with n < 2^R.
 *   1. E = 1 on a COSINE handle (prepared rows have |x| < 2; a group's centroid does not depend on what else matched).
 *      On L2 and IP handles m = the maximum over the considered rows and j < dim of bits(x) & 0x7fffffff, an integer max;
 *      m >= 0x7f800000 -- a considered row holds an infinity or a NaN, which a bf16 handle can round a large finite value
 *      to -- is VROD_ERR_INVALID_ARG; otherwise E = max(m >> 23, 1) - 126, so that max |x| < 2^E.
 *   2. s = 62 - R - E.
 *   3. q = llrint((double)x * 2^s): the product is exact in fp64, ties round to even, |q| <= 2^(62 - R).
 *   4. S = the sum of q over the group's rows in int64: fewer than 2^R rows, so |S| < 2^62 -- it never wraps, and the
 *      sum is exact and commutative.
 *   5. With VROD_CENTROID_SUM the output is (float)((double)S * 2^-s), otherwise
 *      (float)(((double)S / (double)count) * 2^-s): each conversion and the division one IEEE round-to-nearest-even
 *      operation.  S == 0 gives +0.0f.  The mean is not re-normalised under COSINE: the searches normalise their queries.
 * So no bit of the result depends on scheduling, on the order of the rows inside a group or on how partial sums are
 * folded; repeated calls, and two handles holding the same rows in another order, give identical bytes.
 * The _device form leaves the vectors in device memory (stream and pointer rules of vrod_index_get_rows_device), from
 * where vrod_search_device or vrod_index_add_device(VROD_SRC_F32) can take them; the group records and both counts go to
 * host memory in both forms.
 * Refusals, all before the first write (a refused call writes nothing, not even the counts): a null idx, pred,
 * out_count, out_groups or vectors, capacity == 0 or > VROD_MAX_CENTROID_GROUPS, flag bits outside 1u | 8u,
 * out_row_stride < dim or capacity * out_row_stride overflowing, a pending search: VROD_ERR_INVALID_ARG; a multi-device
 * handle: VROD_ERR_UNSUPPORTED; more groups than capacity: VROD_ERR_CAPACITY (size with
 * vrod_index_aggregate_where(limit = 0)).  A predicate that can match nothing, or an empty handle, is VROD_OK with zero
 * groups and no pass.  vrod_index_last_stats and the handle's state are not touched; nothing is persisted. */
#define VROD_CENTROID_SUM 8u       /* flags: write each group's sum, not its mean; shares the word with VROD_ROWPRED_ALLOWED (1u) */
#define VROD_MAX_CENTROID_GROUPS 65536u
typedef struct {
    int64_t  key;
    uint64_t count;       /* rows of the group */
    uint64_t first_id;    /* smallest id of the group, id_offset applied */
} vrod_centroid_group; /* 24 bytes, no padding */
int vrod_index_centroids_where(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags, uint32_t by, int64_t width,
                               uint32_t capacity, uint64_t *out_count, uint64_t *out_rows,
                               vrod_centroid_group *out_groups, float *out_vectors, uint64_t out_row_stride);
int vrod_index_centroids_where_device(vrod_index *idx, const vrod_row_pred *pred, uint32_t flags, uint32_t by, int64_t width,
                                      uint32_t capacity, uint64_t *out_count, uint64_t *out_rows,
                                      vrod_centroid_group *out_groups, float *d_out_vectors, uint64_t out_row_stride,
                                      void *stream);

/* Duplicate rows -- the classes of LIVE rows whose stored form is bit-identical, found in one read of the corpus.
 * Two live rows are duplicates when the dim stored elements of their prepared rows -- what vrod_index_get_rows reads
 * back: 16 bits per element on a BF16 handle, 32 on an F32 handle -- have the same bits.  -0.0 and +0.0 differ.  Under
 * COSINE this is equality after normalisation (x and 2x land in one class), on a BF16 handle equality after rounding.
 * The padding up to the row pitch is never compared.  Searches score prepared rows only, so the rows of one class have
 * identical score bits against every query under every metric: they are the ties a search cannot separate.  Deleted
 * rows belong to no class; the filter is not consulted, as with keys.  With VROD_DUP_WITHIN_LABEL the class key is
 * (label, row bits): equal rows with different labels (the same chunk in two documents or two tenants) are then not
 * duplicates; a handle that never set labels has label 0 everywhere.  A hash only chooses which rows are compared;
 * every class rests on a comparison of the rows themselves, so the result is exact.
 *   find_duplicates   out_first (host memory) may be NULL with map_len == 0, a stats-only call; otherwise map_len must
 *                     equal vrod_index_count (the rule of vrod_index_compact's map), anything else is
 *                     VROD_ERR_INVALID_ARG.  out_first[i] = the smallest id, id_offset applied, among the live rows of the
 *                     class of row offset + i: a row without a copy gets its own id, a deleted row VROD_ID_NONE.  The
 *                     array is a function of the handle's state alone: every call gives the same one.
 *                     *out_stats (may be NULL): live, classes, duplicates and largest_class are exact and
 *                     reproducible; slots, max_probe and compare_misses are DIAGNOSTICS of this call's hash table and
 *                     may differ between calls.
 *   find_duplicates_device  d_out_first is device memory on the handle's device; the stream rules are those of
 *                     vrod_index_find_keys_device (the caller's work on `stream` is complete before the library writes,
 *                     the call returns when the map is in place).  The stats still come back to host memory.
 *   delete_duplicates deletes every live row whose out_first is not its own id, exactly as vrod_index_delete of those ids
 *                     would: tombstones, the dead rows' keys free, vrod_index_filter_count and vrod_index_live_count
 *                     drop.  *out_deleted (may be NULL) = rows that died = stats.duplicates.  THE SURVIVOR OF A CLASS IS
 *                     ITS SMALLEST ID; a caller who wants another rule calls find_duplicates and deletes for themselves.
 *                     Nothing moves: vrod_index_compact reclaims the space as for any delete.
 * VROD_DUP_NARROW_HASH is a diagnostic for tests: the row hash is cut to 8 bits before it is used, so that unequal rows
 * meet in the table on a corpus of a few hundred rows.  Results are identical with and without it.
 * Common rules: single-device handles only -- a multi-device handle answers VROD_ERR_UNSUPPORTED; while a search is
 * pending: VROD_ERR_INVALID_ARG; unknown flag bits: VROD_ERR_INVALID_ARG; an empty handle, or one with no live row:
 * VROD_OK and all-zero stats.  Every check and allocation comes before the first write: a refused call,
 * VROD_ERR_OUT_OF_MEMORY included, leaves outputs and handle untouched.  The table lives in device memory for the length
 * of the call only (44 to 76 bytes per live row); every walk of it is bounded by its slot count, and one that runs out is
 * VROD_ERR_INTERNAL, not a hang.  Nothing is persisted: a snapshot does not change. */
#define VROD_DUP_WITHIN_LABEL 1u
#define VROD_DUP_NARROW_HASH  0x80000000u   /* diagnostic: see above */
typedef struct {
    uint64_t live;            /* live rows looked at */
    uint64_t classes;         /* distinct stored rows among them */
    uint64_t duplicates;      /* live - classes: what vrod_index_delete_duplicates would delete */
    uint64_t largest_class;   /* rows in the largest class, 0 on a handle with no live row */
    uint64_t slots;           /* diagnostic: table size of this call */
    uint64_t max_probe;       /* diagnostic, may differ between calls */
    uint64_t compare_misses;  /* diagnostic: full row comparisons that found a difference */
} vrod_dup_stats;
int vrod_index_find_duplicates(vrod_index *idx, uint32_t flags, uint64_t *out_first, uint64_t map_len,
                               vrod_dup_stats *out_stats);
int vrod_index_find_duplicates_device(vrod_index *idx, uint32_t flags, uint64_t *d_out_first, uint64_t map_len,
                                      vrod_dup_stats *out_stats, void *stream);
int vrod_index_delete_duplicates(vrod_index *idx, uint32_t flags, uint64_t *out_deleted);

/* Row lookup -- "are these vectors in here already?", answered from the rows themselves, and an add that appends only
 * the vectors that are not: the question that comes BEFORE vrod_index_find_duplicates, for callers without keys.
 * Equality.  Input i is first prepared exactly as vrod_index_add would store it: fp16 / bf16 sources are widened, the
 * norm chain and the division run under COSINE, a BF16 handle rounds to bf16.  It EQUALS a stored row when the dim stored
 * elements have the same bits -- the equality of vrod_index_find_duplicates: -0.0 is not +0.0, the padding is never
 * compared, x and 2x are one row under COSINE, an fp32 vector and its bf16-rounded twin are one row on a BF16 handle.
 * Deleted rows are never found; the filter is not consulted, as with keys and find_duplicates.  A hash only chooses
 * which rows are compared; every answer rests on a comparison of the rows themselves, so the result is exact.
 *   find_rows     out_ids[i] (host memory; may be NULL, a stats-only call) = the SMALLEST ID, id_offset applied, among
 *                 the live rows equal to input i, VROD_ID_NONE if there is none.  Inputs may repeat: repeats get the
 *                 same answer.  The handle is not changed in any observable way: a snapshot does not change.
 *   add_unique    in call order: input i with a live stored copy gets that row's smallest id and nothing is appended;
 *                 otherwise, if an earlier input j < i of the same call has the same prepared bits, it gets out_ids[j];
 *                 otherwise it is appended exactly as vrod_index_add would append it -- the next id, no key, the default
 *                 label, tags and value.  Afterwards the handle is what ONE vrod_index_add of just the appended inputs,
 *                 in order, would have left: rows, every search (ids and score bits), the certificate bound, counts and
 *                 the bytes of a snapshot.  The same batch again appends nothing.  out_ids may be NULL.
 *   the _device forms take rows as vrod_index_add_device does (src_dtype, row_stride; the same layout errors) and write
 *                 d_out_ids (may be NULL), device memory on the handle's device.  The stream rules are those of
 *                 vrod_index_find_keys_device: the caller's work on `stream` (may be NULL) is complete before the library
 *                 reads or writes, and the call returns when the ids are in place.  At most 16 bytes per input cross to
 *                 the host; the rows do not.  The stats still come back to host memory.
 *   *out_stats (may be NULL): rows, found, repeats and appended are exact and reproducible; batches, slots, max_probe
 *                 and compare_misses are DIAGNOSTICS of how this call cut its work and of its hash tables, and may differ
 *                 between calls.
 * VROD_ROWFIND_NARROW_HASH and VROD_ROWFIND_SMALL_BATCH are diagnostics for tests: the row hash is cut to 8 bits (as
 * VROD_DUP_NARROW_HASH), the call's lookup batches hold 96 rows.  Results are identical with and without them.
 * Errors: NaN / Inf anywhere in the inputs: VROD_ERR_INVALID_VALUE, every input being checked before the first row is
 * written; unknown flag bits, or a pending search: VROD_ERR_INVALID_ARG; a multi-device handle: VROD_ERR_UNSUPPORTED;
 * n == 0: VROD_OK and all-zero stats.  A refused call, VROD_ERR_OUT_OF_MEMORY included, leaves outputs, rows, norms, the
 * certificate bound, count and key table as they were; spare capacity may have grown.  The corpus is hashed once per call
 * and every batch's table lives in device memory for the length of the call only (8 bytes per stored row and per input,
 * about 50 per row of a batch); every walk of a table is bounded by its slot count, and one that runs out is
 * VROD_ERR_INTERNAL, not a hang.  Nothing is persisted. */
#define VROD_ROWFIND_NARROW_HASH 0x80000000u  /* diagnostic: row hash cut to 8 bits, as VROD_DUP_NARROW_HASH */
#define VROD_ROWFIND_SMALL_BATCH 0x40000000u  /* diagnostic: the call's lookup batches hold 96 rows */
typedef struct {
    uint64_t rows;            /* inputs of the call */
    uint64_t found;           /* inputs whose prepared form a live row stored BEFORE the call */
    uint64_t repeats;         /* inputs without such a row that equal an earlier input of the call */
    uint64_t appended;        /* add_unique: rows - found - repeats; find_rows: 0 */
    uint64_t batches;         /* diagnostic: lookup batches of this call */
    uint64_t slots;           /* diagnostic: size of the largest batch table */
    uint64_t max_probe;       /* diagnostic, may differ between calls */
    uint64_t compare_misses;  /* diagnostic: full row comparisons that found a difference */
} vrod_rowfind_stats;
int vrod_index_find_rows(vrod_index *idx, const float *rows, uint64_t n, uint32_t flags, uint64_t *out_ids,
                         vrod_rowfind_stats *out_stats);
int vrod_index_find_rows_device(vrod_index *idx, const void *d_rows, int src_dtype, uint64_t row_stride, uint64_t n,
                                uint32_t flags, uint64_t *d_out_ids, vrod_rowfind_stats *out_stats, void *stream);
int vrod_index_add_unique(vrod_index *idx, const float *rows, uint64_t n, uint32_t flags, uint64_t *out_ids,
                          vrod_rowfind_stats *out_stats);
int vrod_index_add_unique_device(vrod_index *idx, const void *d_rows, int src_dtype, uint64_t row_stride, uint64_t n,
                                 uint32_t flags, uint64_t *d_out_ids, vrod_rowfind_stats *out_stats, void *stream);

/* Near-duplicate rows -- the classes of ELIGIBLE rows that a score threshold ties together: the re-encoded paragraph,
 * the chunk of a second crawl, a row and its bf16-rounded twin.  The range counterpart of vrod_knn_graph and the
 * similarity counterpart of vrod_index_find_duplicates.
 * Rows.  The ELIGIBLE rows: live and, while a filter is set, allowed -- the rule of every score-based call, and UNLIKE
 * vrod_index_find_duplicates, WHICH IGNORES THE FILTER: vrod_index_set_filter_where + find_near_duplicates is "dedupe
 * within this tenant / predicate".  A row that is not eligible belongs to no class, gets VROD_ID_NONE and is never
 * deleted by these calls.
 * Edge.  Eligible rows i != j are joined when j qualifies for i, or i for j, in the sense of a range search whose query
 * is the prepared row AS STORED (the rule of vrod_search_by_ids: not normalised again, not rounded again) and whose
 * comparison is vrod_range_search's: canonical score s >= threshold (COSINE, IP) or s <= threshold (L2), as fp32
 * values, inclusive; a NaN score never qualifies.  With the canonical chains (left-to-right q*x, or (q-x)^2) the relation
 * is symmetric bit for bit; the definition does not depend on that.  A NaN threshold is VROD_ERR_INVALID_VALUE, +-inf is
 * allowed.
 * Classes.  The connected components of that graph: SINGLE LINKAGE at the threshold.  CHAINING: a~b and b~c put a and c
 * in one class even when a and c do not qualify for each other -- a loose threshold can string a whole corpus together.
 *   find_near_duplicates  out_first (host memory) may be NULL with map_len == 0, a stats-only call; otherwise map_len must
 *                     equal vrod_index_count, anything else is VROD_ERR_INVALID_ARG (the rule of find_duplicates).
 *                     out_first[i] = the smallest id, id_offset applied, among the rows of the class of row offset + i: a
 *                     row with no qualifying neighbour gets its own id, a row that is not eligible VROD_ID_NONE.
 *                     *out_stats (may be NULL): rows, classes, near_duplicates, largest_class and hits are exact.  The
 *                     map and those five are functions of the handle's state and the threshold alone; batches, splits
 *                     and pool_entries are DIAGNOSTICS of how this call cut its work.
 *   find_near_duplicates_device  d_out_first is device memory on the handle's device; the stream rules are those of
 *                     vrod_index_find_duplicates_device.  The stats still come back to host memory.
 *   delete_near_duplicates  deletes every eligible row whose out_first is not its own id, exactly as vrod_index_delete
 *                     of those ids would.  THE SURVIVOR OF A CLASS IS ITS SMALLEST ID.  *out_deleted (may be NULL) =
 *                     rows that died = stats.near_duplicates.  Nothing moves (vrod_index_compact reclaims the space).
 * VROD_NEAR_SMALL_POOL is a diagnostic for tests: the hit pool of the call holds exactly as many entries as there are
 * eligible rows, so that batches are split on a corpus of a few thousand rows.  Results are identical with and without it.
 * Cost.  One scan of the eligible rows per batch of eligible rows (1024 rows of a BF16 handle, 256 of an F32 handle):
 * quadratic in the corpus, as vrod_knn_graph.  It is also at least linear in `hits`, and a LOOSE THRESHOLD MAKES `hits`
 * QUADRATIC TOO: a batch whose hits overflow the call's pool (64 MiB, or 16 bytes per eligible row if that is more) is
 * scanned again in halves.  vrod_index_set_path is honoured as by a range search.
 * Common rules: single-device handles only -- a multi-device handle answers VROD_ERR_UNSUPPORTED; while a search is
 * pending: VROD_ERR_INVALID_ARG; unknown flag bits: VROD_ERR_INVALID_ARG; an empty handle, or one with no eligible row:
 * VROD_OK and all-zero stats.  Every check, and every allocation whose size is known up front, comes before the first
 * write to an output or to the handle.  The union-find lives in device memory for the length of the call (8 bytes per
 * row); its walks are bounded by the row count, and one that runs out is VROD_ERR_INTERNAL, not a hang.  Nothing is
 * persisted: a snapshot does not change. */
#define VROD_NEAR_SMALL_POOL 0x80000000u   /* diagnostic: see above */
typedef struct {
    uint64_t rows;            /* eligible rows looked at */
    uint64_t classes;         /* connected components among them */
    uint64_t near_duplicates; /* rows - classes: what vrod_index_delete_near_duplicates would delete */
    uint64_t largest_class;   /* rows in the largest class, 0 on a handle with no eligible row */
    uint64_t hits;            /* sum over eligible rows i of the OTHER eligible rows j that qualify for i (directed) */
    uint64_t batches;         /* diagnostic: range scans run */
    uint64_t splits;          /* diagnostic: batches redone in halves because their hits overflowed the pool */
    uint64_t pool_entries;    /* diagnostic: hit-pool size of this call */
} vrod_near_stats;
int vrod_index_find_near_duplicates(vrod_index *idx, float threshold, uint32_t flags, uint64_t *out_first, uint64_t map_len,
                                    vrod_near_stats *out_stats);
int vrod_index_find_near_duplicates_device(vrod_index *idx, float threshold, uint32_t flags, uint64_t *d_out_first, uint64_t map_len,
                                           vrod_near_stats *out_stats, void *stream);
int vrod_index_delete_near_duplicates(vrod_index *idx, float threshold, uint32_t flags, uint64_t *out_deleted);

/* Grouped search -- the best row of each label, the k best labels per query (a document stored as many chunk rows that
 * share a label: the k best documents, not k chunks of one).  The ELIGIBLE rows of a query are the rows that are live
 * and, while a filter is set, allowed by the handle's filter.  Every label carried by at least one eligible row has one
 * REPRESENTATIVE, its best eligible row: the best canonical score, ties broken by the smaller id, a NaN score last, as in
 * vrod_search.  Query q's result row is the k best representatives, best first, ties by smaller id, id_offset applied;
 * out_ids / out_scores are nq x k, out_labels (nq x k, may be NULL) holds the label of each result; slots beyond the
 * number of distinct labels are (VROD_ID_NONE, NaN) with label 0.  Scores are the CPU oracle's bits: the row is what the
 * oracle's top-1 over each label's eligible rows, sorted, gives.  A handle whose labels were never set holds label 0 in
 * every row: each query gets exactly one result.  k, null pointers and NaN / Inf in the queries are handled as
 * vrod_search handles them.  Synchronous, like the labelled and range searches: no _begin_ form, no graph replay;
 * VROD_ERR_INVALID_ARG while a search is pending; the _device form takes device pointers and returns after the results
 * are complete in device memory.  Exact for any group size: the ordinary search runs with more results per query (4 k,
 * at least k + 32, at most VROD_MAX_K or the eligible rows) and its lists are de-duplicated by label on the device; a
 * query whose list ends before k labels are found -- a few labels own all of it -- is finished from the canonical scores
 * of every row, with the rows of the labels already taken masked, in as many rounds as it needs (at most k).
 * vrod_index_set_path is honoured by the first search; EXACT sends every query straight to the canonical scores.
 * An empty handle, or one without an eligible row, gives all-unfilled rows without looking at the queries, as
 * vrod_search does.  vrod_index_last_stats afterwards: path = the first search's, or VROD_PATH_EXACT when every query took the canonical
 * scores; k as given; kprime = the first search's; fallback_queries = the first search's + the queries that took the
 * canonical scores; scan_bytes / scan_flops = the first search's + every stored row (x the queries) per pass over the
 * corpus (one per 8 such queries), each such pass one more of scan_launches and part of scan_ms.  Multi-device handles: VROD_ERR_UNSUPPORTED, the outputs are not touched. */
int vrod_search_grouped(vrod_index *idx, const float *queries, uint32_t nq, uint32_t k,
                        uint64_t *out_ids, float *out_scores, uint32_t *out_labels);
int vrod_search_grouped_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k,
                               uint64_t *d_out_ids, float *d_out_scores, uint32_t *d_out_labels, void *stream);

/* Multi-vector search -- a query is a SET of vectors (several phrasings, query tokens, a late-interaction encoder's
 * output), a document the rows that share a label, and each document is scored by MaxSim:
 *     S(q, L) = sum over the query's vectors t, first to last, of M(t, L),
 *     M(t, L) = the best canonical score of vector t over the ELIGIBLE rows of label L (live, and allowed while a filter is
 *               set): the maximum for COSINE and IP, the minimum for L2; a NaN row score loses to any number, M is NaN only
 *               if every eligible row of L scores NaN.
 * S is an fp32 sum taken left to right from +0.0f, one rounding per add; under IP overflow it may be +-inf or NaN.
 *   vectors     query_lims[nq] x dim fp32; every vector is prepared exactly as vrod_search prepares a query (normalised for
 *               COSINE, bf16-rounded on BF16 handles); NaN or Inf anywhere: VROD_ERR_INVALID_VALUE.
 *   query_lims  nq + 1 words: query q owns vectors [query_lims[q], query_lims[q + 1]).  query_lims[0] != 0, a decreasing
 *               entry, a query with 0 or with more than VROD_MAX_QUERY_VECTORS vectors: VROD_ERR_INVALID_ARG.
 *   result      row q of out_labels / out_scores (nq x k) holds the k best labels among those with at least one eligible
 *               row -- the highest S for COSINE and IP, the lowest for L2, a NaN S last, ties by the smaller label -- and
 *               their S; out_found[q] (out_found may be NULL) = the filled slots = min(k, labels with an eligible row); the
 *               slots past it are (label 0, NaN).  Score bits are the CPU oracle's: its top-1 over each label's eligible
 *               rows per vector, added in fp32 in order (a NaN matches any NaN).
 * Labels are those of vrod_index_set_labels; a handle whose labels were never set is one document with label 0.  Tags are
 * ignored.  k and null pointers are handled as vrod_search_grouped handles them; nq == 0: VROD_OK.  Every check comes before
 * the first write: a refused call leaves the outputs untouched.  An empty handle, or one without an eligible row, gives
 * all-unfilled rows without looking at the vectors, as vrod_search does.  Synchronous: no _begin_ form, no graph replay;
 * VROD_ERR_INVALID_ARG while a search is pending; the _device form takes device pointers on the handle's device (query_lims
 * included) and returns after the results are complete in device memory.  Multi-device handles: VROD_ERR_UNSUPPORTED, the
 * outputs are not touched.
 * Exact by one of two routes per query.  Candidate route: the ordinary certified search runs for every vector with k1
 * results each (the grouped search's rule; a call with more than 2048 vectors is cut between queries); the labels of the
 * rows in a query's lists are its candidates, the eligible rows of the candidates are scored against the query's vectors
 * and S is ranked among them.  With theta_t the last score of vector t's full list, a label outside every list has
 * M(t, L) no better than theta_t, and rounded addition is monotone, so U = the same fp32 sum of the theta_t bounds S of
 * every other label: the answer stands when the query has k candidates and its k-th S is strictly better than U, or when
 * one of its lists came back short (then every label is a candidate).  Dense route, for every other query -- a list with
 * a NaN or infinite score, candidates that own more than a quarter of the rows, a failed certificate -- and for every
 * query under VROD_PATH_EXACT or on a handle without labels: the canonical scores of every row, folded to the best per
 * (vector, document) and added per document.  vrod_index_set_path is honoured by the first-stage search.
 * vrod_index_last_stats afterwards, as after vrod_search_grouped: path = the first search's, or VROD_PATH_EXACT when every
 * query went dense; nq = the queries (not the vectors); k as given; kprime = the first search's; fallback_queries = the
 * first search's + the dense queries; scan_bytes / scan_flops = the first search's + the rows (x the vectors) of every
 * candidate label scored + every stored row (x the query's vectors) per dense pass over the corpus (one per 8 vectors of a
 * dense query), each such launch one more of scan_launches; scan_ms stays the first search's.
 * vrod_index_last_multivec: what the last multi-vector call did -- which route answered (certified_queries + dense_queries
 * = nq), k1 (0 when no first-stage search ran), and the candidate labels and rows scored, summed over the queries. */
#define VROD_MAX_QUERY_VECTORS 256u
typedef struct {
    uint32_t nq, vectors, k1, certified_queries, dense_queries;
    uint64_t candidate_labels, candidate_rows;
} vrod_multivec_stats;
int vrod_search_multivec(vrod_index *idx, const float *vectors, const uint32_t *query_lims, uint32_t nq, uint32_t k,
                         uint32_t *out_labels, float *out_scores, uint32_t *out_found);
int vrod_search_multivec_device(vrod_index *idx, const float *d_vectors, const uint32_t *d_query_lims, uint32_t nq, uint32_t k,
                                uint32_t *d_out_labels, float *d_out_scores, uint32_t *d_out_found, void *stream);
int vrod_index_last_multivec(const vrod_index *idx, vrod_multivec_stats *out);

/* Diversified search -- exact greedy Maximal Marginal Relevance over the certified top pool: the answer to "the ten rows
 * are ten copies of the same thing" when nobody has labelled the copies.  Per query:
 *   pool       what vrod_search returns for it with k = pool over the eligible rows (live, and allowed while a filter is
 *              set): positions 0 .. m-1, best first, m = the filled slots (m <= pool), r_i = the canonical score at
 *              position i.  Labels and tags are ignored.
 *   pair score g(i, j) = the canonical score between the PREPARED stored rows at positions i and j, used as stored, exactly
 *              as vrod_search_by_ids scores a stored row against another (the chain is symmetric in its operands for all
 *              three metrics).
 *   redundancy pen_i = the best g(i, s) over the rows s selected so far -- the maximum for COSINE and IP, the minimum for
 *              L2, folded in selection order, an equal g changing nothing; a NaN g loses to any number, pen_i is NaN only
 *              if every such g is NaN.
 *   selection  step 0 takes position 0.  Step t >= 1 evaluates every position i not selected yet, with mu = fl(1 - lambda):
 *                  v_i = fl( fl(lambda * r_i) - fl(mu * pen_i) )
 *              every operation rounded once to fp32, no fused multiply-add, and takes the largest v for COSINE and IP, the
 *              smallest for L2; values compare as fp32 (-0.0 == +0.0), a NaN v loses to any number, ties -- an all-NaN step
 *              included -- go to the smaller pool position.  min(k, m) steps.
 *   result     row q of out_ids / out_scores / out_mmr (nq x k) lists the selected rows in SELECTION order: the id
 *              (id_offset applied), r_i -- the oracle's bits -- and v at the moment of selection, slot 0 holding
 *              fl(lambda * r_0); out_mmr may be NULL.  Slots past min(k, m) are (VROD_ID_NONE, NaN, NaN).
 * lambda = 1 reproduces vrod_search's first k bit for bit on finite scores; lambda = 0 ranks by redundancy alone.
 * k = 0, k > pool, pool > VROD_MAX_DIVERSE_POOL, lambda NaN or outside [0, 1], null pointers: VROD_ERR_INVALID_ARG; NaN or
 * Inf in the queries: VROD_ERR_INVALID_VALUE, as vrod_search; nq == 0: VROD_OK.  Every check comes before the first write: a
 * refused call leaves the outputs untouched.  An empty handle, or one without an eligible row, gives all-unfilled rows
 * without looking at the queries.  Synchronous: no _begin_ form, no graph replay; VROD_ERR_INVALID_ARG while a search is
 * pending; the _device form takes device pointers and returns after the results are complete in device memory.
 * Multi-device handles: VROD_ERR_UNSUPPORTED, the outputs are not touched.
 * The first stage is the ordinary certified search with `pool` results (vrod_index_set_path is honoured by it); one more
 * launch then selects on the device, a work-group per query with its state in LDS, scoring the pool against each newly
 * selected row with the canonical chain: k * m chains, never the m x m matrix.  vrod_index_last_stats afterwards reports
 * the first-stage search, with k = the caller's k. */
#define VROD_MAX_DIVERSE_POOL 1024u
int vrod_search_diverse(vrod_index *idx, const float *queries, uint32_t nq, uint32_t k, uint32_t pool, float lambda,
                        uint64_t *out_ids, float *out_scores, float *out_mmr);
int vrod_search_diverse_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k, uint32_t pool, float lambda,
                               uint64_t *d_out_ids, float *d_out_scores, float *d_out_mmr, void *stream);

/* Search by stored row id ("more like this") -- query q is the PREPARED stored row ids[q] (nq ids as searches report
 * them, id_offset applied; host memory, the _device form: device memory), used as stored: it is not normalised again and
 * not rounded again, so the scores are scores between stored rows and an L2 row is at distance +0.0 from itself.  The
 * result row is bit for bit (ids and score bits, a NaN matching any NaN) the CPU oracle's canonical scan of that prepared
 * row over the ELIGIBLE rows (live, and allowed while a filter is set): best first, ties by smaller id, slots beyond the
 * eligible rows (VROD_ID_NONE, NaN).  Labels are ignored, as in vrod_search.  flags: 0, or VROD_BYID_EXCLUDE_SELF: row
 * ids[q] is not a candidate of query q -- the result is the top k of the eligible rows other than itself.  The drop is by
 * id, not by position: an exact duplicate with a smaller id ranks before the row itself, under IP the row need not be its
 * own best match, under a filter it may not be eligible at all.  With the flag k may be at most VROD_MAX_K - 1 (the
 * search runs with k + 1 results); a larger k, and unknown flag bits: VROD_ERR_INVALID_ARG.  An id may repeat.  An id that
 * is not a current row, or names a deleted row, fails the whole call with VROD_ERR_INVALID_ARG and the outputs are not
 * touched (the _device form: the launch that gathers the rows checks every id and raises one flag, read before anything
 * else runs -- no host copy of the ids).  nq == 0: VROD_OK.  Synchronous: no _begin_ form, no graph replay;
 * VROD_ERR_INVALID_ARG while a search is pending; the _device form takes device pointers and returns after the results are
 * complete in device memory.  vrod_index_set_path is honoured as by vrod_search.  vrod_index_last_stats afterwards: what
 * the underlying search reported, k = the caller's k.  Multi-device handles: VROD_ERR_UNSUPPORTED, the outputs are not
 * touched. */
enum { VROD_BYID_EXCLUDE_SELF = 1u };
int vrod_search_by_ids(vrod_index *idx, const uint64_t *ids, uint32_t nq, uint32_t k, uint32_t flags,
                       uint64_t *out_ids, float *out_scores);
int vrod_search_by_ids_device(vrod_index *idx, const uint64_t *d_ids, uint32_t nq, uint32_t k, uint32_t flags,
                              uint64_t *d_out_ids, float *d_out_scores, void *stream);
/* The exact k-NN graph of the corpus: for every row with id in [first_id, first_id + n), result row i (out_ids /
 * out_scores: host memory, n x k) holds the k nearest OTHER eligible rows of id first_id + i -- exactly what
 * vrod_search_by_ids(.., VROD_BYID_EXCLUDE_SELF) returns for that id.  A DELETED row in the range gets an all-unfilled
 * result row ((VROD_ID_NONE, NaN) in every slot) and is never scanned for: the range form stays usable between a delete
 * and a compact.  A filter that is set restricts the neighbours, not the queries.  A range that is not wholly within the
 * current rows: VROD_ERR_INVALID_ARG; k at most VROD_MAX_K - 1; n == 0: VROD_OK.  The library cuts the range into batches
 * of its own choosing and keeps two in flight: batch s + 1's gather and scan are
 * enqueued before batch s's lists lose self and are copied out; the results do not depend on the batch size.
 * vrod_index_last_stats afterwards: nq = the live rows of the range, k as given, scan_launches / scan_bytes / scan_flops /
 * scan_ms / fallback_queries / band_queries = sums over the batches, kprime / max_fast_err / eps_bound = maxima, path =
 * the last batch's.  VROD_ERR_INVALID_ARG while a search is pending; multi-device handles: VROD_ERR_UNSUPPORTED, the
 * outputs are not touched. */
int vrod_knn_graph(vrod_index *idx, uint64_t first_id, uint64_t n, uint32_t k,
                   uint64_t *out_ids, float *out_scores);

/* Search by weighted examples ("more like these, less like those, never what was seen") -- the query is combined on the
 * device from an optional vector and stored rows, and the result leaves a per-query set of ids out.  Per query q, with
 * fl() one rounding to fp32 and no fused multiply-add anywhere:
 *   operands     If `vectors` is given (nq x dim; may be NULL), row q of it is the first operand: prepared first exactly as
 *                vrod_search prepares a query (normalised for COSINE, bf16-rounded on BF16 handles), with weight
 *                vector_weights[q], or 1.0f when that pointer is NULL.  The terms term_ids[term_lims[q] .. term_lims[q + 1])
 *                follow in the order given (term_lims: nq + 1 entries, term_ids / term_weights: term_lims[nq] entries): each
 *                is the PREPARED stored row as vrod_index_get_rows returns it -- bf16 widened, nothing normalised or rounded
 *                again -- with weight term_weights[t].  Term ids are ids as searches report them, id_offset applied.
 *   combination  For each coordinate j: acc = +0.0f, then for each operand in order acc = fl(acc + fl(w * x[j])).  The order
 *                is part of the contract.
 *   search       The combined vector is a raw query to vrod_search: prepared again (normalised for COSINE, bf16-rounded on
 *                BF16) and searched over the eligible rows (live, and allowed while a filter is set).  Labels and tags are
 *                ignored; vrod_index_set_path is honoured.
 *   exclusion    The excluded set of q is exclude_ids[exclude_lims[q] .. exclude_lims[q + 1]) (both NULL: none) and, with
 *                VROD_COMBINED_EXCLUDE_TERMS, q's term ids.  The result is the top k of the eligible rows outside that set:
 *                best first, ties by smaller id, slots beyond it (VROD_ID_NONE, NaN).  Exclusion is by id; an excluded id
 *                that is not a current row, names a deleted row, repeats, or equals VROD_ID_NONE is ignored: seen-lists
 *                outlive deletes.
 * The result is bit for bit what the CPU oracle gives for the combined vector over those rows.
 * Every check comes before the first write: a refused call leaves the outputs untouched.  VROD_ERR_INVALID_ARG: null
 * required pointers; term_lims[0] != 0 or a decreasing entry, the same for exclude_lims; a query with no operand at all (no
 * vector and zero terms); more than VROD_MAX_COMBINE_TERMS terms in a query; more than VROD_MAX_EXCLUDE excluded entries in
 * a query (its terms included under the flag, duplicates counted); unknown flag bits; k == 0; k + the batch's largest
 * excluded count > VROD_MAX_K (the search runs with that many results); a term id that is not a live row (the host form
 * checks its mirror of the tombstones; the _device form: the launch that combines checks every id and raises one flag, read
 * before the search is begun); a pending search.  VROD_ERR_INVALID_VALUE: NaN or Inf in `vectors` or in a weight, or a
 * combined vector that holds a NaN or Inf (overflow).  Multi-device handles: VROD_ERR_UNSUPPORTED.  nq == 0: VROD_OK.  An
 * empty handle, or one without an eligible row, gives all-unfilled rows, as vrod_search does.
 * Synchronous: no _begin_ form, no graph replay; the _device form takes device pointers (the two lims arrays are copied
 * to the host) and returns after the results are complete in device memory.  vrod_index_last_stats afterwards: what the
 * underlying search reported, k = the caller's k. */
#define VROD_MAX_COMBINE_TERMS 256u    /* stored-row operands per query */
#define VROD_MAX_EXCLUDE 1024u         /* excluded ids per query: the terms under the flag + its exclude list */
enum { VROD_COMBINED_EXCLUDE_TERMS = 1u };
int vrod_search_combined(vrod_index *idx, const float *vectors, const float *vector_weights,
                         const uint32_t *term_lims, const uint64_t *term_ids, const float *term_weights,
                         const uint32_t *exclude_lims, const uint64_t *exclude_ids,
                         uint32_t nq, uint32_t k, uint32_t flags, uint64_t *out_ids, float *out_scores);
int vrod_search_combined_device(vrod_index *idx, const float *d_vectors, const float *d_vector_weights,
                                const uint32_t *d_term_lims, const uint64_t *d_term_ids, const float *d_term_weights,
                                const uint32_t *d_exclude_lims, const uint64_t *d_exclude_ids,
                                uint32_t nq, uint32_t k, uint32_t flags, uint64_t *d_out_ids, float *d_out_scores, void *stream);

/* Candidate-list searches -- the second stage of hybrid retrieval: the caller already holds a list of ids per query (from a
 * keyword index, an SQL pre-filter, an access-control lookup) and wants only those rows scored.
 *   lists           Query q owns cand_ids[cand_lims[q] .. cand_lims[q + 1]) (cand_lims: nq + 1 entries, cand_ids:
 *                   cand_lims[nq] entries, in any order).  Ids are ids as searches report them, id_offset applied.
 *   candidate set   The DISTINCT ids of q's list that are current rows, live, and allowed by the handle's filter while one
 *                   is set.  An id below the offset, past the count, equal to VROD_ID_NONE, deleted or disallowed is
 *                   ignored, not an error, and a repeated id counts once: lists kept outside the database outlive deletes
 *                   (the rule of vrod_search_combined's exclude lists).  Labels and tags are ignored.
 * vrod_search_candidates: result row q (out_ids / out_scores: nq x k) is bit for bit -- ids and score bits, a NaN matching
 * any NaN -- what vrod_search returns for that query on a fresh handle that holds only the candidate rows, in ascending id
 * order, with the ids mapped back: best first, ties by smaller id, NaN last, whatever the order of the caller's list.  Slots
 * beyond the candidate set are (VROD_ID_NONE, NaN); an empty list, or one with nothing eligible in it, gives an
 * all-unfilled row.  k ranges over 1 .. VROD_MAX_K.
 * vrod_score_candidates: out_scores has cand_lims[nq] entries aligned with cand_ids; entry t of query q is the canonical
 * score of q against row cand_ids[t] -- the bits vrod_search would report for that row -- and NaN where the id is ignored
 * under the rule above.  A repeated id gets its score at every position.  Under IP a score whose terms overflow to +inf and
 * -inf is NaN as well: the two cases cannot be told apart here.
 * Queries are prepared exactly as vrod_search prepares them; NaN / Inf in them: VROD_ERR_INVALID_VALUE.
 * VROD_ERR_INVALID_ARG: null required pointers; cand_lims[0] != 0 or a decreasing entry; a list of more than
 * VROD_MAX_CANDIDATES entries (repeats and ignored ids counted); k == 0 or k > VROD_MAX_K; a pending search.  Every check
 * comes before the first write: a refused call leaves the outputs untouched.  Multi-device handles: VROD_ERR_UNSUPPORTED,
 * the outputs are not touched.  nq == 0: VROD_OK.  An empty handle, or one without an eligible row, gives all-unfilled rows
 * (the search form) or all NaN (the score form) without looking at the queries.
 * Synchronous: no _begin_ form, no graph replay; the _device forms take device pointers (cand_lims included: it is copied
 * to the host to be checked, the ids never are) and return after the results are complete in device memory.
 * vrod_index_set_path is ignored: the candidates are always scored on their own rows by the canonical chain, there is no
 * fast pass and no certificate.  vrod_index_last_stats afterwards: path = VROD_PATH_GATHER, nq, k (0 for the score form),
 * kprime = the largest candidate set of the batch (the score form: the most entries scored for one query, repeats
 * counted), scan_launches = the score launches, fallback_queries = band_queries = 0, max_fast_err = eps_bound = 0,
 * scan_bytes = the rows scored x the stored row bytes and scan_flops = 2 x the rows scored x dim, summed over the queries
 * (the search form scores a candidate set once, the score form every eligible entry, repeats included). */
#define VROD_MAX_CANDIDATES 16384u   /* list entries per query, repeats and stale ids counted */
int vrod_search_candidates(vrod_index *idx, const float *queries, uint32_t nq, uint32_t k,
                           const uint32_t *cand_lims, const uint64_t *cand_ids,
                           uint64_t *out_ids, float *out_scores);
int vrod_search_candidates_device(vrod_index *idx, const float *d_queries, uint32_t nq, uint32_t k,
                                  const uint32_t *d_cand_lims, const uint64_t *d_cand_ids,
                                  uint64_t *d_out_ids, float *d_out_scores, void *stream);
int vrod_score_candidates(vrod_index *idx, const float *queries, uint32_t nq,
                          const uint32_t *cand_lims, const uint64_t *cand_ids, float *out_scores);
int vrod_score_candidates_device(vrod_index *idx, const float *d_queries, uint32_t nq,
                                 const uint32_t *d_cand_lims, const uint64_t *d_cand_ids, float *d_out_scores, void *stream);

/* Merge n_lists per-shard results (device, each nq x k, list-major: [list][q][k]) into
 * one nq x k on `device` -- the step after the RCCL all-gather. */
int vrod_merge_topk_device(int device, int metric, const uint64_t *d_ids,
                           const float *d_scores, uint32_t n_lists, uint32_t nq,
                           uint32_t k, uint64_t *d_out_ids, float *d_out_scores,
                           void *stream);

/* Same merge over ONE packed buffer: per list, nq*k ids (u64) immediately followed by nq*k
 * scores (f32) -- the layout that lets the exchange be a single all-gather. nq*k must be even. */
int vrod_merge_topk_packed_device(int device, int metric, const void *d_packed, uint32_t n_lists,
                                  uint32_t nq, uint32_t k, uint64_t *d_out_ids,
                                  float *d_out_scores, void *stream);

/* --- knobs & introspection --------------------------------------------------
 * Environment, read when a handle is created: VROD_F32_SPLIT.  An F32 handle keeps bf16
 * [hi | lo] planes of its rows (a second copy of the corpus, built at the first batched search)
 * and runs batched searches as three bf16 matrix-core products instead of one fp32 one (2.5x
 * faster at 10M x 1536, batch 256); the results are the same bits: only the fast pass and the
 * certificate's bound change.  Default: on while the planes leave max(1/8 of the device, 4 GiB)
 * free, and switched off for the handle after two searches in which more than 1/8 of the queries
 * failed the (wider) certificate.  =0: never.  =1: always (no margin check, never switched off).
 * If the planes cannot be allocated the handle quietly keeps the fp32 pass. */
int vrod_index_set_path(vrod_index *idx, int path);      /* VROD_PATH_* (default AUTO) */
int vrod_index_set_profiling(vrod_index *idx, int on);   /* 1: scan_ms (events attached to the scan dispatches), 2: + total_ms (stream markers) */
int vrod_index_last_stats(const vrod_index *idx, vrod_search_stats *out);
/* The same counters for ONE shard of the most recently completed search (a multi-device handle has a shard per
 * entry of device_ids, in that order; a single-device handle has shard 0 = itself), and the device the shard
 * lives on (out_device may be NULL): what each GPU of such a handle spent.  shard out of range: INVALID_ARG. */
int vrod_index_shard_stats(const vrod_index *idx, uint32_t shard, int *out_device, vrod_search_stats *out);
const char *vrod_last_error(void);                       /* thread-local text */
const char *vrod_version(void);

/* --- synthetic stream on the device (tests: bit-parity with the oracle) ----- */
int vrod_synth_rows_device(int device, uint64_t seed, uint64_t first_row, uint64_t n,
                           uint32_t dim, float *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VROD_H */
