/*
 * mqvs.h -- C-ABI of libmqvs.so, the MI355X (gfx950) vector-scan engine that
 * sits behind MyScaleDB's brute-force distance() path.
 *
 * Every entry point is plain C (pointers, sizes, ints); no HIP, torch or C++
 * types cross this boundary.  The reference-side C++ binding that a MyScaleDB
 * maintainer drops in is include/mqvs_vector_index.hpp.
 *
 * Reference interfaces replaced (paths relative to the MyScaleDB tree):
 *   mqvs_knn_raw        VectorIndex::tryBruteForceSearch<FloatVector>
 *                       src/VectorIndex/Common/BruteForceSearch.h:62-111
 *   mqvs_segment_*      the per-granule copy of the Array(Float32) column into
 *                       `vector_raw_data` + VectorDataset construction,
 *                       src/VectorIndex/Storages/MergeTreeVSManager.cpp:1366-1393,
 *                       src/VectorIndex/Common/VectorDataset.h:31-60
 *                       (a whole data part is registered once and stays in HBM)
 *   mqvs_search         MergeTreeVSManager::vectorScanWithoutIndex<Float> +
 *                       searchWrapper + VIWithColumnInPart::searchWithoutIndex,
 *                       MergeTreeVSManager.cpp:960-1680, VIWithDataPart.h:341-382
 *   mqvs_rerank         VIWithColumnInPart::computeTopDistanceSubset,
 *                       src/VectorIndex/Common/VIWithDataPart.cpp:838-856
 *   mqvs_merge_shards   MergeTreeBaseSearchManager::getTotalTopSearchResultImpl,
 *                       src/VectorIndex/Storages/MergeTreeBaseSearchManager.cpp:207-297
 *                       (and the Distributed engine's shard merge)
 *   mqvs_last_error /   DB::Exception(code, message) thrown by the above
 *   status codes        (ErrorCodes NOT_IMPLEMENTED, LOGICAL_ERROR, ...)
 *
 * Threading: re-entrant.  Each calling thread gets its own HIP stream and
 * scratch workspace; segments are read-only after creation and may be searched
 * from any number of threads (the reference admits 2 x physical cores
 * concurrent scans, MergeTreeVSManager.cpp:974-975).
 */
#ifndef MQVS_H
#define MQVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQVS_ABI_VERSION 4

/* Metric ids (VICommon.h VIMetric).  L2 / IP / Cosine: Float32 vectors;
 * Hamming / Jaccard: binary vectors (FixedString(N) columns, mqvs_*_binary). */
enum {
    MQVS_METRIC_L2 = 0,      /* squared L2, ascending */
    MQVS_METRIC_IP = 1,      /* inner product, descending */
    MQVS_METRIC_COSINE = 2,  /* 1 - <q/|q|, y/|y|>, ascending */
    MQVS_METRIC_HAMMING = 4, /* popcount(q ^ y), ascending (value 3 is internal) */
    MQVS_METRIC_JACCARD = 5  /* (|q|y| - |q&y|) / |q|y| in fp32, ascending */
};

/* Status codes; each maps 1:1 onto the DB::ErrorCodes the reference throws. */
enum {
    MQVS_OK = 0,
    MQVS_ERR_NOT_IMPLEMENTED = 1,   /* unsupported metric (BruteForceSearch.h:89) */
    MQVS_ERR_LOGICAL = 2,           /* dim mismatch, wrong segment metric (LOGICAL_ERROR) */
    MQVS_ERR_ILLEGAL_COLUMN = 3,    /* malformed column data */
    MQVS_ERR_BAD_ARGUMENTS = 4,     /* null pointers, k <= 0, ... */
    MQVS_ERR_MEMORY_LIMIT = 5,      /* HBM allocation failed (MEMORY_LIMIT_EXCEEDED) */
    MQVS_ERR_DEVICE = 6,            /* HIP runtime / kernel failure */
    MQVS_ERR_CHECKSUM = 7           /* compressed block checksum mismatch (CHECKSUM_DOESNT_MATCH) */
};

/* mqvs_search / mqvs_rerank flags */
#define MQVS_F_DEVICE_PTRS 0x1u /* queries, bitmaps, candidates and outputs are
                                   device pointers on the segment's GPU */
#define MQVS_F_ASYNC 0x2u       /* with DEVICE_PTRS: do not synchronise the
                                   stream before returning.  The results are
                                   valid once the stream drains AND
                                   mqvs_async_check returns MQVS_OK: a search
                                   that would have needed a host-driven
                                   fallback (candidate overflow, a query whose
                                   norm is NaN, infinite or >= 1e18 on a
                                   pre-filtered segment, cosine variant
                                   check) is reported there as
                                   MQVS_ERR_LOGICAL and must be repeated
                                   without ASYNC */
/* Per-call path selection (override the process-wide mqvs_set_* defaults for
 * this call only; all paths return the same bits): */
#define MQVS_F_EXACT 0x20u         /* exact fp32 scan of every row (no bf16 pre-filter) */
#define MQVS_F_GATHER_NEVER 0x40u  /* PREWHERE: scan every row and mask */
#define MQVS_F_GATHER_ALWAYS 0x80u /* PREWHERE: always walk a gather list of the selected rows */
#define MQVS_F_TIMING 0x100u       /* per-launch HIP-event timing in mqvs_last_search_stats */

typedef struct mqvs_segment *mqvs_segment_t;
typedef struct mqvs_index *mqvs_index_t; /* an index over a resident segment (index path, below) */
typedef void *mqvs_stream_t; /* a hipStream_t, or NULL for the caller thread's stream */

/* ---- lifecycle ---------------------------------------------------------- */
int mqvs_abi_version(void);
/* Bind the calling thread to `device` (a HIP ordinal). */
int mqvs_init(int device);
int mqvs_device_count(int *count);
/* Thread-local message of the last failing call on this thread. */
const char *mqvs_last_error(void);
/* Outcome of this thread's MQVS_F_ASYNC calls on the current device since the
 * last check: synchronises `stream` (NULL: the thread's own stream), then
 * returns MQVS_OK, or MQVS_ERR_LOGICAL when one of them needed a host-driven
 * fallback (its results are then invalid: repeat it synchronously).  Clears
 * the record.  Callers that used several streams synchronise them first. */
int mqvs_async_check(mqvs_stream_t stream);
/* Release this thread's streams and workspaces -- the FLAT search workspace
 * and the index search workspace (its scratch, events and the side stream of
 * the cosine variant chain) -- after their last searches' kernels finish
 * (optional; a pool thread that retires should call it). */
int mqvs_thread_release(void);
/* Library shutdown for the calling thread (SURVEY 8(b) lifecycle): waits for
 * the thread's streams and releases its workspaces, as mqvs_thread_release.
 * Segments, indexes, caches and communicators stay owned by the caller and
 * are freed with their own *_free calls. */
int mqvs_shutdown(void);

/* ---- segments: one data part's Array(Float32) column resident in HBM ---- */
/* host_rows: n*d row-major fp32; rows whose Array is empty must be FLT_MAX
 *   filled (MergeTreeVSManager.cpp:1381) and flagged 0 in `nonempty`.
 * nonempty: n bytes (1 = non-empty array) or NULL (all non-empty).
 * metric: the column's metric; COSINE segments are normalised in HBM once
 *   (VectorDataset.h:98-117 per row) and serve only cosine searches; L2/IP
 *   segments serve both L2 and IP.
 * granule_rows: index_granularity (rows per mark; reads are chunked by it).
 * row_offset: id of row 0 (0 for a whole part; shard start for a row-range
 *   shard of a part -- must be a multiple of granule_rows). */
int mqvs_segment_create(const float *host_rows, int64_t n, int32_t d, int32_t metric,
                        int64_t granule_rows, const uint8_t *nonempty, int64_t row_offset,
                        mqvs_segment_t *out);
/* Same from a device buffer on the current device (copied). */
int mqvs_segment_create_device(const float *dev_rows, int64_t n, int32_t d, int32_t metric,
                               int64_t granule_rows, const uint8_t *dev_nonempty,
                               int64_t row_offset, mqvs_segment_t *out);
/* Synthetic segment generated in HBM by the counter-based generator
 * (mode 0 exact ints in [-8,8], 1 ~N(0,1), 2 Gaussian mixture of 4096 centres
 * with noise 0.25, 3 "hard" mixture of 65536 centres with noise 1.0); row r of the
 * segment is generator row row_offset + r. */
int mqvs_segment_generate(uint64_t seed, int32_t mode, int64_t n, int32_t d, int32_t metric,
                          int64_t granule_rows, int64_t row_offset, mqvs_segment_t *out);
int mqvs_segment_free(mqvs_segment_t seg);
int mqvs_segment_info(mqvs_segment_t seg, int64_t *n, int32_t *d, int32_t *metric,
                      int64_t *granule_rows, int64_t *row_offset, size_t *hbm_bytes);
/* The segment's pre-filter planes: *split = 2 (the bf16 plane, see
 * mqvs_set_prefilter) or 0 when the planes were off or did not fit in HBM --
 * batches then run the exact fp32 MFMA path over every row (same bits, about
 * 1/16 of the bf16 MFMA rate); *plane_bytes = their HBM bytes (included in
 * mqvs_segment_info's hbm_bytes); *approx_ok = 1 when the pre-filter serves
 * searches (planes present and the rows' norms finite and moderate). */
int mqvs_segment_prefilter(mqvs_segment_t seg, int32_t *split, size_t *plane_bytes, int32_t *approx_ok);
/* Where the segment's Float32 rows live.  host = 1 moves them to pinned host
 * memory mapped into the device's address space: HBM then holds the bf16
 * pre-filter plane, the norms and the maps (2 B per element instead of 6), so
 * a part about 3x larger fits.  Searches keep the same pipeline and return the
 * same bits; the exact re-rank reads its survivors' rows over PCIe (a few
 * hundred rows per query), while paths that read every row (no plane, no
 * pre-filter, mqvs_set_batch_mode(1), index build) stream the whole part over
 * PCIe: correct, slow.  host = 0 moves the rows back into HBM.  The caller
 * keeps searches on the segment from running meanwhile, and changes the
 * residency before handing the segment to the part cache (its weight is
 * taken at put).  *host (mqvs_segment_rows_host) = 1 when the rows are in host
 * memory.  (No reference counterpart: MyScaleDB re-reads the column from disk
 * per search, MergeTreeVSManager.cpp:1348-1393.) */
int mqvs_segment_set_rows_host(mqvs_segment_t seg, int32_t host);
int mqvs_segment_rows_host(mqvs_segment_t seg, int32_t *host);
/* Device pointer of the resident rows (normalised rows for cosine). */
int mqvs_segment_rows(mqvs_segment_t seg, const float **dev_rows);

/* ---- search --------------------------------------------------------------
 * Brute-force top-k over the whole segment, with the reference operator's
 * exact output: k (id, distance) per query, ascending for L2/Cosine,
 * descending for IP, ties by row order; ids are row_offset + row; slots past
 * the last result hold id -1 and distance FLT_MAX (L2, Cosine) or FLT_MIN (IP).
 * queries: nq*d fp32 (original, un-normalised).
 * filter: PREWHERE bitmap, LSB-first, n bits, or NULL (no PREWHERE).
 * row_exists: lightweight-delete mask, LSB-first, n bits (1 = live), or NULL.
 * out_ids: nq*k int64; out_dist: nq*k fp32 (caller-owned).
 * k: 1 .. 16384 (the reference's max_search_result_window is 10000,
 * Settings.h:923); above 4096 the final sort runs through a device scratch
 * and large batches are searched in query sub-batches. */
int mqvs_search(mqvs_segment_t seg, const float *queries, int32_t nq, int32_t k,
                int32_t metric, const uint8_t *filter, const uint8_t *row_exists,
                int64_t *out_ids, float *out_dist, uint32_t flags, mqvs_stream_t stream);

/* mqvs_search for a row-range shard of a part, with the cosine chunk-ordinal
 * base given: the number of granule chunks BEFORE the shard's first row that
 * the reference searches for this query (MergeTreeVSManager.cpp:960-1536:
 * a chunk is searched iff it holds a non-empty row that, with a PREWHERE
 * filter, also passes the filter and is not deleted).  The query is
 * re-normalised once per searched chunk, so this base picks the variant.
 * chunk_ord_base < 0: row_offset / granule_rows (every earlier chunk
 * searched).  Only cosine results depend on it. */
int mqvs_search_ex(mqvs_segment_t seg, const float *queries, int32_t nq, int32_t k, int32_t metric,
                   const uint8_t *filter, const uint8_t *row_exists, int64_t chunk_ord_base,
                   int64_t *out_ids, float *out_dist, uint32_t flags, mqvs_stream_t stream);

/* tryBruteForceSearch contract (BruteForceSearch.h:62-111): x nx*d queries,
 * y ny*d base (host pointers), one pass with no granule chunking, metric L2 or
 * IP only (anything else -> MQVS_ERR_NOT_IMPLEMENTED); result_id / distance
 * nx*k, faiss layout (-1 / FLT_MAX or -FLT_MAX padding). */
int mqvs_knn_raw(const float *x, const float *y, int64_t d, int64_t k, int64_t nx, int64_t ny,
                 int32_t metric, int64_t *result_id, float *distance);

/* Exact re-rank of candidate rows (computeTopDistanceSubset contract,
 * VIWithDataPart.cpp:838-856): cand is nq*ncand segment-local row ids (-1 or
 * out-of-range = none; distinct rows per query), ncand <= 32768, k <= 16384
 * (above 4096 candidates the records are sorted through global scratch).  Each
 * candidate gets the distance mqvs_search computes for the same batch size
 * (nq < 20 sequential formula, else BLAS form; cosine with the row's chunk
 * query variant); rows cleared in row_exists (LSB-first, n bits, or NULL)
 * are skipped.  Output: top-k as mqvs_search (same order key and padding). */
int mqvs_rerank(mqvs_segment_t seg, const float *queries, int32_t nq, const int64_t *cand,
                int32_t ncand, int32_t k, int32_t metric, const uint8_t *row_exists,
                int64_t *out_ids, float *out_dist, uint32_t flags, mqvs_stream_t stream);

/* Merge per-list top-k results: in_ids/in_dist [nshards][nq][k] as returned
 * by mqvs_search; out nq*k (nshards * k <= 2^20; above 4096 the records are
 * sorted through a device scratch of 32 B per record and query).
 * Default (row-range shards of ONE part, shard s holding lower ids than shard
 * s+1): order distance (desc for IP), then shard, then position -- the result
 * equals the unsharded part's search.
 * MQVS_F_PART_MERGE (lists = different data parts): the reference's cross-part
 * merge MergeTreeBaseSearchManager::getTotalTopSearchResultImpl
 * (MergeTreeBaseSearchManager.cpp:207-297), an insertion-ordered multimap read
 * backwards for IP -- equal IP scores come out last-inserted first. */
#define MQVS_F_PART_MERGE 0x4u
int mqvs_merge_shards(int32_t nshards, int32_t nq, int32_t k, int32_t metric,
                      const int64_t *in_ids, const float *in_dist, int64_t *out_ids,
                      float *out_dist, uint32_t flags, mqvs_stream_t stream);

/* ---- part groups: many small resident parts searched in one fused call
 * The parts of a MergeTree table that have no index yet (fresh inserts, recent
 * merges) are many and small; the reference scans them with one thread per
 * part (MergeTreeSelectWithHybridSearchProcessor.cpp:1212-1241) and merges the
 * per-part top-k in getTotalTopSearchResultImpl
 * (MergeTreeBaseSearchManager.cpp:207-297).  A group is an ordered list of
 * Float32 segments -- the list order is the part order of that merge, the
 * reference's insertion order -- and mqvs_part_group_search returns, for every
 * input, exactly what
 *     mqvs_search(segs[p], queries, nq, k, metric, filters[p], row_exists[p])
 *         for every p (the same nq, so the same faiss formula branch), then
 *     mqvs_merge_shards(nparts, ..., MQVS_F_PART_MERGE) over the lists in
 *         group order
 * returns: ids, distance bits, order and padding (id -1, FLT_MAX, or FLT_MIN
 * for IP) match bit for bit.  out_part[q][i] is the position in the group of
 * the part result i came from (-1 in padding slots): the caller reads the
 * winning rows from that part.
 *
 * The group borrows the segments (they outlive it; the cache and the caller
 * keep ownership).  Creation is cheap: it validates and remembers the handles,
 * copies no rows and makes no pass over them, so a caller may build a group
 * per query as its set of parts changes.  The per-part descriptors (rows
 * pointer, n, granule, row offset, chunk ordinals and non-empty bitmap, tile
 * and column prefix sums, the call's bitmaps) are taken from the live segments
 * by every search and uploaded as one small table with it: a segment may move
 * its rows between HBM and host memory (mqvs_segment_set_rows_host) while a
 * group holds it, and the group itself holds no device memory (hbm_bytes 0).
 * Errors of mqvs_part_group_create: nparts < 1, a null handle, or segments on
 * different devices -> MQVS_ERR_BAD_ARGUMENTS; binary and Float32 segments
 * mixed, differing dimensions (binary: differing dim_bits), or cosine and
 * non-cosine Float32 segments mixed -> MQVS_ERR_LOGICAL.  A group whose
 * segments are all binary (FixedString) is searched by
 * mqvs_part_group_search_binary, below; mqvs_part_group_search on it is
 * MQVS_ERR_LOGICAL.
 * mqvs_part_group_info: rows = the sum of the parts' rows; d = the dimension
 * (binary: dim_bits); fusable_parts = the parts whose rows are in HBM and
 * number at most the part-group row limit (binary: the binary row limit).
 *
 * mqvs_part_group_search.  filters / row_exists: host arrays of nparts
 * pointers; either array may be NULL, any entry may be NULL; each bitmap
 * (LSB-first) covers its own part's rows.  With MQVS_F_DEVICE_PTRS the
 * queries, the three outputs and every bitmap are device pointers (the two
 * pointer arrays stay host arrays).  MQVS_F_ASYNC is ignored: the call always
 * ends with the merged result, after one host wait (as the sharded calls).
 * nparts * k > 2^20 -> MQVS_ERR_BAD_ARGUMENTS (the merge's limit); a metric
 * the segments were not prepared for -> MQVS_ERR_LOGICAL.  The call honours
 * mqvs_inject_fault as mqvs_search does (outputs untouched) and its scratch
 * passes the workspace budget gate, counted in the thread's workspace.
 * Three routes, the same bits on all of them:
 *   fused     nq < 20, k <= 4096, and the part has its rows in HBM and at most
 *             the part-group row limit of them: all such parts are searched by
 *             one query prep, one grouped exact fp32 scan (dense values), one
 *             grouped select and the merge -- a launch chain whose length
 *             does not depend on nparts (a group whose dense [nq][rows] matrix
 *             passes mqvs_set_scratch_budget runs scan + select per slice of
 *             parts).  Every row of a part is a candidate of its select, so no
 *             candidate list can overflow and no part is ever re-run (redo
 *             stays 0).  Cosine: the query variant table is sized for the part
 *             with the most chunk ordinals (up to 16384, within the scratch
 *             budget), so a chain that does not repeat needs no second run.
 *   fused     nq >= 20, off unless mqvs_set_part_group_batch has set a row
 *   batch     limit: then k <= 4096, nq at most the setting's max_nq (when it
 *             has one), and the part has its rows in HBM and at most the batch
 *             row limit of them.  The same chain as the fused route -- one
 *             query prep (with |q|^2 for L2), per slice of parts one grouped
 *             scan and one grouped select, the merge, one host wait -- on the
 *             exact fp32 MFMA scan of faiss's BLAS formula branch (128-row
 *             tiles, the dense matrix [nq][rows] fp32 sliced by
 *             mqvs_set_scratch_budget).  No overflow, no re-run (redo 0); the
 *             cosine variant table is sized as on the fused route.
 *   per part  every other part and call (k > 4096, rows in host memory,
 *             larger parts, nq >= 20 with the batch route off or past its
 *             max_nq; on both fused routes also a cosine part that carries a
 *             PREWHERE filter, whose chunk ordinals come from the filter, and
 *             a cosine part of more chunk ordinals than the variant table may
 *             hold): mqvs_search's own path on the same stream; the list
 *             joins the same merge.
 * mqvs_set_part_group_rows: the row limit of the fused route (default 131072,
 * the largest measured part size at which the fused route still beat the
 * per-part one at nq 1 and nq 16, profiles/part_group; at most 2^24); returns
 * the previous value, 0 leaves it unchanged.
 * mqvs_set_part_group_batch: rows = 0 turns the fused batch route off (the
 * default: every call then takes the routes, launches and stats it took
 * before the route existed); 1 .. 2^24 is its row limit.  max_nq = 0: no cap
 * on nq, else a cap >= 20.  Other values: MQVS_ERR_BAD_ARGUMENTS, nothing
 * changed.  mqvs_part_group_batch reads the pair (either pointer may be NULL).
 * Recommended when batches arrive over many small parts: (131072, 128), the
 * largest measured pair at which the fused batch route beat the per-part one
 * at every measured nq up to max_nq (20, 128), for L2 and cosine, in groups
 * of 8 equal parts (profiles/part_group, "Batches"); at nq 1000 it wins for
 * 64 parts of 8192 rows and 256 of 1000 but loses for 8 parts of 16384 or
 * 32768 rows, where the per-part route's bf16 pre-filter is faster.
 *
 * Binary part groups.  A group of binary segments (all of one dim_bits, on one
 * device; a segment's default metric does not matter, a binary segment serves
 * Hamming and Jaccard) holds the parts of a FixedString(N) column that have no
 * BINARYMSTG index yet.  mqvs_part_group_search_binary returns, for every
 * input, exactly what
 *     mqvs_search_binary(segs[p], queries, nq, k, metric, filters[p],
 *         row_exists[p]) for every p, then
 *     mqvs_merge_shards(nparts, ..., MQVS_F_PART_MERGE) over the lists in
 *         group order
 * returns: ids (row_offset + row), distance bits and order (ascending by
 * distance, then part, then position in the part's list) match bit for bit;
 * padding slots hold id -1 and FLT_MAX, and out_part the group position of
 * each result, -1 in padding slots.  queries: nq x dim_bits / 8 bytes.  The
 * bitmaps, the pointer arrays, MQVS_F_DEVICE_PTRS and MQVS_F_ASYNC (ignored:
 * one host wait, after the merge) are as in mqvs_part_group_search; so are
 * the nparts * k limit, mqvs_inject_fault, the workspace gate and the stats
 * (mqvs_part_group_last_stats, batch = 0).  A metric other than Hamming /
 * Jaccard -> MQVS_ERR_NOT_IMPLEMENTED; the call on a Float32 group ->
 * MQVS_ERR_LOGICAL.
 * Two routes, the same bits on both:
 *   fused     k <= 4096 and the part has its codes in HBM and at most the
 *             binary row limit of them, at any nq (binary distances have no
 *             formula switch at nq 20): the query codes are uploaded once,
 *             then per slice of parts (the dense [nq][rows] fp32 matrix cut by
 *             mqvs_set_scratch_budget) one grouped popcount scan -- the dense
 *             values of mqvs_search_binary's own scans: the Hamming count, the
 *             fp32 Jaccard (den - num) / den, NaN for a row that is filtered,
 *             deleted or at Hamming distance dim_bits -- and one grouped
 *             select, then the merge.  Every row of a part is a candidate of
 *             its select: nothing overflows, redo stays 0.  A filter never
 *             sends a part to the other route (no chunk ordinals here).
 *   per part  everything else (k > 4096, larger parts): mqvs_search_binary's
 *             own path on the same stream; the list joins the same merge.
 * mqvs_set_part_group_binary_rows: the binary row limit (default 131072, the
 * largest measured part size at which the fused route beat the per-part one
 * at nq 1, 16 and 128 for both metrics, profiles/part_group/binary_limit.jsonl
 * -- up to 32768 rows mqvs_search_binary itself scans the whole part into
 * dense values, so there the fused route does the same device work with fewer
 * launches and waits; at most 2^24); returns the previous value, 0 leaves it
 * unchanged. */
typedef struct mqvs_part_group *mqvs_part_group_t;
int mqvs_part_group_create(const mqvs_segment_t *segs, int32_t nparts, mqvs_part_group_t *out);
int mqvs_part_group_free(mqvs_part_group_t group);
int mqvs_part_group_info(mqvs_part_group_t group, int32_t *nparts, int64_t *rows, int32_t *d,
                         int32_t *fusable_parts, size_t *hbm_bytes);
int mqvs_part_group_search(mqvs_part_group_t group, const float *queries, int32_t nq, int32_t k, int32_t metric,
                           const uint8_t *const *filters, const uint8_t *const *row_exists,
                           int32_t *out_part, int64_t *out_ids, float *out_dist,
                           uint32_t flags, mqvs_stream_t stream);
int mqvs_part_group_search_binary(mqvs_part_group_t group, const uint8_t *queries, int32_t nq, int32_t k,
                                  int32_t metric, const uint8_t *const *filters, const uint8_t *const *row_exists,
                                  int32_t *out_part, int64_t *out_ids, float *out_dist,
                                  uint32_t flags, mqvs_stream_t stream);
/* Stats of the calling thread's last mqvs_part_group_search / _search_binary. */
typedef struct {
    double total_ms;      /* host time of the call (only with mqvs_set_timing(1) or MQVS_F_TIMING) */
    int64_t fused_rows;   /* rows of the fused parts */
    int32_t parts;
    int32_t fused_parts;
    int32_t looped_parts; /* parts searched by the per-part route */
    int32_t launches;     /* kernel launches the call queued for the fused route and the merge
                             (the per-part searches' own launches are not counted) */
    int32_t redo;         /* fused parts re-run per part (always 0: see above) */
    int32_t nq;
    int32_t k;
    int32_t batch;        /* 1 when the call's fused parts ran the fused batch route (the MFMA scan) */
} mqvs_part_group_stats;
int mqvs_part_group_last_stats(mqvs_part_group_stats *out);
int64_t mqvs_set_part_group_rows(int64_t rows);
int64_t mqvs_set_part_group_binary_rows(int64_t rows);
int mqvs_set_part_group_batch(int64_t rows, int32_t max_nq);
int mqvs_part_group_batch(int64_t *rows, int32_t *max_nq);

/* ---- index groups: many binary indexed parts in one fused call
 * The parts of a table that carry a BINARYMSTG index (mqvs_index_build, below)
 * are searched one by one by the reference and merged
 * (MergeTreeSelectWithHybridSearchProcessor.cpp:1212-1241,
 * MergeTreeBaseSearchManager.cpp:207-297).  An index group is an ordered list
 * of binary indexes -- the list order is the part order of the merge -- and
 * mqvs_index_group_search_binary returns, for every input, exactly what
 *     mqvs_index_search_binary(indexes[p], queries, nq, k, params_p,
 *         filters[p], row_exists[p]) for every p, then
 *     mqvs_merge_shards(nparts, ..., MQVS_F_PART_MERGE) over the lists in
 *         group order
 * returns: ids (row_offset + row, then the part's row-ids map), distance bits
 * and order (ascending by distance, then part, then position in the part's
 * list) match bit for bit; padding slots hold id -1 and FLT_MAX, and out_part
 * the group position of each result, -1 in padding slots.
 * params_p is params with one change: an explicit nprobe (1..4096) is replaced
 * by min(nprobe, nlist of part p) -- the parts of one table differ in their
 * list counts, and mqvs_index_search_binary refuses nprobe > nlist; a part
 * whose nprobe reaches its nlist is searched exhaustively.  Without nprobe each
 * part resolves its own from alpha, as its own call does.  metric: one search
 * metric for all parts (default: the first index's); num_reorder is accepted
 * and ignored; an unknown key -> MQVS_ERR_BAD_ARGUMENTS.
 *
 * The group borrows the indexes and their segments (keep them alive while it
 * is used); it copies nothing, makes no device pass and holds no device memory
 * (hbm_bytes = 0).  Every search reads the live indexes, so a row-ids map
 * registered after mqvs_index_group_create is honoured.
 * Errors of mqvs_index_group_create: nparts < 1, a null handle, or indexes on
 * different devices -> MQVS_ERR_BAD_ARGUMENTS; indexes of different dim_bits ->
 * MQVS_ERR_LOGICAL; a Float32 index in the list -> MQVS_ERR_NOT_IMPLEMENTED
 * (float index groups are not built).
 * mqvs_index_group_info: rows = the sum of the segments' rows; lists = the sum
 * of the indexes' nlist.  Any output pointer may be NULL.
 *
 * queries: nq x dim_bits / 8 bytes.  filters / row_exists: host arrays of
 * nparts pointers to packed bitmaps (bit r % 8 of byte r / 8 = row r of the
 * part); either array, or any entry, may be NULL.  With MQVS_F_DEVICE_PTRS the
 * queries, the outputs and the bitmaps the entries point to are device
 * pointers (the arrays themselves stay on the host).  MQVS_F_ASYNC is ignored
 * (one host wait, after the merge); MQVS_F_FIRST_STAGE is accepted and returns
 * the same result.  k: 1..16384; nparts * k > 2^20 -> MQVS_ERR_BAD_ARGUMENTS.
 * mqvs_inject_fault is honoured (the outputs untouched), the call has a wait
 * history of its own, and its scratch lives in the thread's workspace, behind
 * the workspace budget gate.
 * Two routes, the same bits on both:
 *   fused     k <= 4096 and the part's scratch -- nq x (cap_p x 8 +
 *             (nprobe_p < nlist_p ? 4 nlist_p : 0)) bytes, cap_p =
 *             min(nprobe_p x max_list_p, npos_p) records per query -- fits
 *             mqvs_set_scratch_budget, at any nq.  The query codes are
 *             uploaded once; the fused parts are cut into slices whose summed
 *             scratch fits the budget; per slice one grouped centroid-distance
 *             kernel, one grouped pick, one grouped list scan and one grouped
 *             select; then one grouped id map (only if a fused part has a
 *             row-ids map), one stats kernel, the merge and one host wait.
 *             The launch count does not depend on nparts.  A record region
 *             holds every position of its probed lists: nothing overflows and
 *             nothing is re-run.
 *   per part  everything else (k > 4096, a part whose own scratch passes the
 *             budget): mqvs_index_search_binary's own path on the same stream
 *             with the resolved nprobe (it sub-batches the queries); the list
 *             joins the same merge. */
typedef struct mqvs_index_group *mqvs_index_group_t;
int mqvs_index_group_create(const mqvs_index_t *indexes, int32_t nparts, mqvs_index_group_t *out);
int mqvs_index_group_free(mqvs_index_group_t group);
int mqvs_index_group_info(mqvs_index_group_t group, int32_t *nparts, int64_t *rows, int32_t *dim_bits,
                          int64_t *lists, size_t *hbm_bytes);
int mqvs_index_group_search_binary(mqvs_index_group_t group, const uint8_t *queries, int32_t nq, int32_t k,
                                   const char *params, const uint8_t *const *filters,
                                   const uint8_t *const *row_exists, int32_t *out_part, int64_t *out_ids,
                                   float *out_dist, uint32_t flags, mqvs_stream_t stream);
/* Stats of the calling thread's last mqvs_index_group_search_binary. */
typedef struct {
    double total_ms;      /* host time of the call (only with mqvs_set_timing(1) or MQVS_F_TIMING) */
    int64_t values;       /* sums over the fused parts of the per-part index stats */
    int64_t items;        /*   (mqvs_index_search_stats): records kept, non-empty work items, */
    int64_t plane_bytes;  /*   list-plane bytes of the probed lists, (query, list) pairs */
    int64_t pairs;
    int32_t parts;
    int32_t fused_parts;
    int32_t looped_parts; /* parts searched by the per-part route */
    int32_t launches;     /* kernel launches the call queued for the fused route and the merge
                             (the per-part searches' own launches are not counted) */
    int32_t nq;
    int32_t k;
} mqvs_index_group_stats;
int mqvs_index_group_last_stats(mqvs_index_group_stats *out);

/* ---- column ingest: a part's Array(Float32) column from its compressed files
 * Replaces the per-granule host read + copy of vectorScanWithoutIndex
 * (MergeTreeVSManager.cpp:1348-1393): data_bin = the bytes of the nested
 * Float32 stream (`<column>.bin`), sizes_bin = the array sizes stream
 * (`<column>.size0.bin`, UInt64 per row), both as ClickHouse writes them
 * (CompressedWriteBuffer blocks: 16-B checksum, method 0x82 LZ4 or 0x02 NONE,
 * UInt32 compressed size, UInt32 decompressed size, payload).  Every block's
 * checksum -- CityHash128 v1.0.2 of header + payload -- is verified on the GPU
 * first (CompressedReadBufferBase.cpp:37-45, 192-196) unless flags has
 * MQVS_F_NO_CHECKSUM (the reference's disable_checksum).  Decoded on the GPU into the rows of :1381-1393 (FLT_MAX fill;
 * empty arrays flagged empty; arrays longer than d truncated, shorter ones
 * FLT_MAX-padded) and prepared as mqvs_segment_create.  flags:
 * MQVS_F_DEVICE_PTRS when the streams are already in HBM.  Errors:
 * MQVS_ERR_CHECKSUM (a block checksum does not match: CHECKSUM_DOESNT_MATCH),
 * MQVS_ERR_ILLEGAL_COLUMN (malformed blocks, sizes that do not match the data
 * stream or n), MQVS_ERR_NOT_IMPLEMENTED (other codecs). */
#define MQVS_F_NO_CHECKSUM 0x10u
int mqvs_segment_create_from_column(const uint8_t *data_bin, int64_t data_bytes, const uint8_t *sizes_bin,
                                    int64_t sizes_bytes, int64_t n, int32_t d, int32_t metric, int64_t granule_rows,
                                    int64_t row_offset, uint32_t flags, mqvs_segment_t *out);

/* ---- binary vectors: FixedString(N) columns, Hamming / Jaccard ----------
 * tryBruteForceSearch<BinaryVector> (BruteForceSearch.h:94-110) over
 * vectorScanWithoutIndex<BinaryVector> (MergeTreeVSManager.cpp:1188-1273,
 * 1395-1425).  Codes are n rows x dim_bits/8 bytes (the FixedString bytes).
 *
 * mqvs_segment_create_binary: register a part's binary column (host codes, or
 * device codes with MQVS_F_DEVICE_PTRS in flags); metric is the column's
 * default (Hamming or Jaccard; a search may use either).
 * mqvs_search_binary: mqvs_search for binary segments -- queries nq x N bytes;
 * output ascending by (distance, row), Hamming distances as float values
 * (KAT 00038 prints 4, 8, ...), -1 / FLT_MAX padding.  Rows at Hamming
 * distance == dim_bits are never returned (hammings_knn_mc emits b < nBit).
 * mqvs_knn_binary_raw: the tryBruteForceSearch<BinaryVector> contract itself
 * (host pointers, one pass): Hamming writes int32 counts into `distance`
 * (reinterpret as int32_t*, padding -1 / INT32_MAX, faiss::hammings_knn_mc);
 * Jaccard writes floats (padding -1 / FLT_MAX).  Float metrics ->
 * MQVS_ERR_NOT_IMPLEMENTED ("Metric not implemented in brute force search
 * for Binary Vector"), as BruteForceSearch.h:107.
 *
 * mqvs_set_binary_batch (process-wide, off by default): min_nq >= 1 sends
 * every binary brute-force search of nq >= min_nq -- mqvs_search_binary,
 * mqvs_knn_binary_raw, the per-part legs of binary part groups -- through the
 * i8 MFMA scan instead of the popcount scan: the code bits as 0/1 bytes on
 * v_mfma_i32_16x16x64_i8 give popcount(x & q) exactly, and both distances are
 * integer expressions of it, so ids and distance bits do not change.  0 turns
 * the route off; a negative value is MQVS_ERR_BAD_ARGUMENTS and leaves the
 * setting unchanged.  Read once per call.  mqvs_binary_batch reads the setting
 * (min_nq may be NULL). */
int mqvs_set_binary_batch(int32_t min_nq);
int mqvs_binary_batch(int32_t *min_nq);
int mqvs_segment_create_binary(const uint8_t *codes, int64_t n, int32_t dim_bits, int32_t metric,
                               int64_t granule_rows, int64_t row_offset, uint32_t flags,
                               mqvs_segment_t *out);
int mqvs_search_binary(mqvs_segment_t seg, const uint8_t *queries, int32_t nq, int32_t k, int32_t metric,
                       const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                       uint32_t flags, mqvs_stream_t stream);
int mqvs_knn_binary_raw(const uint8_t *x, const uint8_t *y, int64_t d, int64_t k, int64_t nx, int64_t ny,
                        int32_t metric, int64_t *result_id, float *distance);

/* ---- multi-GPU: one part sharded by row range over the GPUs of a node ----
 * One rank per GPU (process or thread); rank r holds the granule-aligned row
 * range [r0, r1) of the part as a segment created with row_offset = r0 (ids
 * stay part-global).  The communicator is an RCCL one over xGMI:
 *   mqvs_comm_unique_id  on ONE rank; ship the 128 bytes to the others out of
 *                        band (the Distributed engine's channel, MPI, a file)
 *   mqvs_comm_init       on every rank, with its device current (mqvs_init);
 *                        blocks until all nranks have joined
 *   mqvs_sharded_search  on every rank, same queries / k / metric: the local
 *                        top-k of the rank's shard, ONE all-gather of the
 *                        per-rank (id, distance) lists (nq*k*12 B per rank),
 *                        and the device merge by (distance, rank, position);
 *                        every rank gets the merged result, bit-identical to
 *                        mqvs_search over the whole part.  filter / row_exists
 *                        are the shard's bitmaps (its n bits).  Cosine: the
 *                        ranks also all-gather how many granule chunks of
 *                        their range the reference searches, which fixes each
 *                        shard's query re-normalisation count (chunk-ordinal
 *                        base) exactly, filters and deletes included.
 * Replaces the cross-part / cross-shard merges of the reference
 * (MergeTreeBaseSearchManager.cpp:207-297 getTotalTopSearchResultImpl; the
 * Distributed engine's per-shard LIMIT + initiator merge,
 * StorageDistributed.cpp:1057-1060) for one part spread over GPUs.  A
 * communicator serves one search at a time.  Before any search work the
 * ranks exchange a header (shard rows, granule, dimension, nq / k / metric,
 * argument errors): shards out of row order, disagreeing calls or a failing
 * rank make EVERY rank return the error instead of leaving the others in a
 * collective; a rank whose local search fails still joins the exchange, and
 * all ranks then fail together.
 * Host syncs: a call equal to the last call every rank completed together
 * (same shard, nq, k, metric and bitmap presence) synchronises the host ONCE
 * (header, local search, exchange and merge enqueued back to back; the
 * exchanged table is read at the end).  The first call, a changed call, or a
 * call whose local search needs a host-driven fallback or whose cosine
 * chunk-ordinal bases changed (filters that empty whole chunks) runs the
 * validated path: header exchange and sync, local search, exchange and sync.
 * MQVS_F_ASYNC is ignored (the call always ends with the merged result). */
#define MQVS_COMM_ID_BYTES 128
typedef struct mqvs_comm *mqvs_comm_t;
int mqvs_comm_unique_id(uint8_t *id /* MQVS_COMM_ID_BYTES */);
int mqvs_comm_init(int32_t nranks, int32_t rank, const uint8_t *id, mqvs_comm_t *out);
int mqvs_comm_free(mqvs_comm_t comm);
/* A loopback communicator group: nranks (<= 64) virtual ranks of ONE process
 * on the current device, out[0 .. nranks-1] one handle per rank.  Each rank's
 * mqvs_sharded_search runs on its own thread (the exchanges are device copies
 * between host barriers); everything else is the RCCL communicator's code.
 * For tests and single-GPU rehearsal of a multi-GPU layout; free every handle. */
int mqvs_comm_init_loopback(int32_t nranks, mqvs_comm_t *out);
int mqvs_sharded_search(mqvs_comm_t comm, mqvs_segment_t shard, const float *queries, int32_t nq, int32_t k,
                        int32_t metric, const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids,
                        float *out_dist, uint32_t flags, mqvs_stream_t stream);
/* The index search of a part sharded by row range: every rank calls it with
 * ITS OWN index, built (mqvs_index_build) or loaded (mqvs_index_load) over
 * its shard segment.  Each rank keeps its own lists; nothing is shared
 * between the ranks' builds, so nprobe counts lists of the rank's index (a
 * part of R ranks probes R * nprobe lists in all).  All ranks pass the same
 * queries, k, params string and MQVS_F_FIRST_STAGE / MQVS_F_RERANK_ALL bits;
 * filter / row_exists are the shard's bitmaps.  The protocol is
 * mqvs_sharded_search's (header, one exchange of the lists, device merge,
 * fast and validated path, every rank returns a failing rank's error); only
 * the local step differs: mqvs_index_search_ex of the rank's index with its
 * exact cosine chunk-ordinal base, taken from the exchanged chunk counts.
 * Every rank gets the merge, bit-identical to mqvs_merge_shards (row-range
 * order) over the ranks' mqvs_index_search_ex results: ids (a registered
 * row-ids map applied by each rank to its own list), distance bits (the
 * approximate ones with MQVS_F_FIRST_STAGE), -1 padding.  When every rank's
 * search is exhaustive (nprobe = its nlist, num_reorder >= its candidates)
 * that is mqvs_search over the whole part, bit for bit.
 * Ranks that disagree on the kind of call (FLAT or index), params or the two
 * flag bits fail everywhere with MQVS_ERR_BAD_ARGUMENTS; a binary index fails
 * everywhere with MQVS_ERR_LOGICAL; an index on another device than the
 * communicator fails alone with MQVS_ERR_BAD_ARGUMENTS.  A communicator
 * serves FLAT and index calls in any order (a change of kind runs the
 * validated path).  MQVS_F_ASYNC is ignored; mqvs_index_last_stats on a rank
 * reports its local search.
 * Not covered: mqvs_rerank takes no base, so a sharded TWO-STAGE cosine
 * search (MQVS_F_FIRST_STAGE here, mqvs_rerank per shard) under filters that
 * empty whole chunks stays the caller's problem. */
int mqvs_sharded_index_search(mqvs_comm_t comm, mqvs_index_t idx, const float *queries, int32_t nq, int32_t k,
                              const char *params, const uint8_t *filter, const uint8_t *row_exists,
                              int64_t *out_ids, float *out_dist, uint32_t flags, mqvs_stream_t stream);
/* Calls of this communicator (FLAT and index) that took the one-sync fast
 * path, and how many of those were re-run on the validated path. */
int mqvs_comm_stats(mqvs_comm_t comm, int64_t *fast_calls, int64_t *redo_calls);

/* Fill a device buffer with generator rows [row0, row0+n) (for queries). */
int mqvs_generate_device(uint64_t seed, int32_t mode, int64_t row0, int64_t n, int32_t d,
                         float *dev_out, mqvs_stream_t stream);

/* ---- index path: MSTG-type vector index over a resident segment ----------
 * The reference's index seam for one data part and vector column:
 *   mqvs_index_build   Search::createVectorIndex<IStream, OStream, DenseBitmap,
 *                      FloatVector>(name, IndexType::MSTG, metric, dim, total_vec,
 *                      params, ...) + VectorIndex::build(...)
 *                      (src/VectorIndex/Common/VIWithDataPart.cpp:416-447,
 *                      VIWithDataPart.h:295-339)
 *   mqvs_index_search  VectorIndex::search(queries, k, params, first_stage_only,
 *                      filter) as VIWithColumnInPart::search calls it
 *                      (VIWithDataPart.cpp:858-957, the call at :926)
 *   computeTopDistanceSubset (stage 2 of a two-stage search,
 *                      VIWithDataPart.cpp:838-856) is mqvs_rerank on the
 *                      index's segment.
 * The MSTG library is absent from the reference snapshot; this
 * is a GPU-native index with its parameter surface: a k-means partition of the
 * part into lists stored as one bf16 plane in list order, an MFMA scan of the
 * lists each query probes, and an exact fp32 re-rank of the best num_reorder
 * candidates (distances bit-identical to mqvs_search / mqvs_rerank for the
 * same rows).
 * The segment must outlive the index.  index_type: "MSTG" (also accepted:
 * "IVFFLAT").  params: comma-separated key=value (Search::Parameters):
 *   metric_type  L2 | IP | Cosine (must match the segment's metric family;
 *                default: the segment's metric)
 *   alpha        default search alpha (MSTG's accuracy knob, [1, 4], default 3)
 *   nlist        lists (default about n / 256, at most 65536)
 *   kmeans_iters k-means iterations (default 8)
 *   sample       k-means training rows (default min(n, max(16 nlist, min(64 nlist, 2^20))))
 *   plane        bf16 | fp8 (case-insensitive; default bf16): the number format
 *                of the list plane, below; any other value fails with
 *                MQVS_ERR_BAD_ARGUMENTS
 * Unknown keys fail with MQVS_ERR_BAD_ARGUMENTS.
 * plane=fp8 stores the list plane at 1 byte per element (OCP e4m3fn codes with
 * one power-of-two scale per list position) instead of 2, so the index takes
 * about half the HBM and a list scan streams half the bytes.  The quantiser,
 * per row y at a list position p (and per query, once per search): amax = max
 * |y_i|; if amax is finite and non-zero, E = the frexp exponent of amax (amax
 * = m 2^E, m in [0.5, 1)) and e_p = 8 - E, else e_p = 0; the stored code of y_i
 * is e4m3fn(y_i 2^e_p), rounded to nearest even (scaled magnitudes lie in
 * [128, 256), under e4m3's 448; a scaled value that is not finite is stored
 * as the NaN code); padding positions and columns >= dim are zero codes.  The
 * approximate inner product of a row and a query is acc 2^-(e_p + e_q), scaled
 * in one exact step, where acc is the fp32 MFMA sum of the code products, each
 * exact in fp32 (the scan widens the codes to bf16, which holds every e4m3
 * value, and sums with the bf16 MFMA: the fp8 MFMA of an MI355X keeps about 13
 * bits under the largest product of an instruction); L2 is
 * (|q|^2 + |y|^2) - 2 ip with the exact fp32 norms.  Only the candidate set
 * and the size of the re-rank's pruning bound change: every returned distance
 * is still the exact fp32 one, and a search that probes every list with
 * num_reorder candidates enough returns mqvs_search's bits.  The coarse
 * quantizer (centroids, mqvs_index_probes) stays bf16 / fp32: an fp8 index
 * probes the lists the bf16 index over the same centroids probes.  A build
 * that chooses nlist from the data (no nlist, >= 2^20 rows) measures np95 by
 * searching the index it built, so with plane=fp8 it measures the fp8 plane.
 * The width limit is shared by both formats (the same bf16 query tile).
 * Width limit: the list scan keeps a tile of 16, 32 or 64 bf16 queries in LDS,
 * 16 QB (2 dpad + 16) + 256 QB bytes for 16 QB queries (dpad: the dimension
 * rounded up to 64), and uses the largest tile that fits the device's
 * per-workgroup LDS.  With the 160 KiB of an MI355X workgroup 64-query tiles
 * serve dpad <= 1216, 32-query tiles dpad <= 2496 and 16-query tiles
 * dpad <= 5056; a segment of more dimensions than that (5056 there) is
 * refused with MQVS_ERR_BAD_ARGUMENTS and a message naming the limit. */
int mqvs_index_build(mqvs_segment_t seg, const char *index_type, const char *params, mqvs_index_t *out);
int mqvs_index_free(mqvs_index_t idx);
typedef struct {
    int64_t nlist;        /* lists */
    int64_t npos;         /* positions of the list-ordered plane (with padding) */
    int64_t max_list;     /* longest list */
    int64_t rows_indexed; /* rows in some list (empty arrays are not indexed) */
    int32_t metric;
    int32_t dim;
    size_t hbm_bytes;     /* index-owned HBM (the segment's rows not counted) */
    double build_ms;
} mqvs_index_info_t;
int mqvs_index_info(mqvs_index_t idx, mqvs_index_info_t *out);
/* The list plane of a float index: *format = MQVS_INDEX_PLANE_BF16 or
 * MQVS_INDEX_PLANE_FP8 (build parameter `plane`), *plane_bytes = the HBM bytes
 * of the list plane (npos x dpad elements of 2 or 1 bytes) plus, for fp8, its
 * per-position scale exponents (int16: 2 npos bytes); mqvs_index_info's
 * hbm_bytes counts them.  Either output may be NULL.  A binary index fails
 * with MQVS_ERR_LOGICAL. */
#define MQVS_INDEX_PLANE_BF16 0
#define MQVS_INDEX_PLANE_FP8 1
int mqvs_index_plane(mqvs_index_t idx, int32_t *format, size_t *plane_bytes);
/* Search params (comma-separated key=value, may be NULL or ""):
 *   alpha        [1, 4]: probes nprobe(alpha) lists (more = higher recall; alpha 3:
 *                max(4, nlist / 256, lists of 4096 rows), doubling per unit)
 *   nprobe       lists probed per query (overrides alpha; <= min(nlist, 4096))
 *   num_reorder  candidates re-ranked exactly (default max(2k, 64), capped at
 *                4096 for k <= 2048; k .. 32768; above 4096 the select and the
 *                re-rank sort through device scratch, 2 num_reorder records of
 *                16 B per query each, in query sub-batches of <= 1 GB)
 * k: 1 .. 16384, as mqvs_search (max_search_result_window, Settings.h:923).
 * filter / row_exists: LSB-first bitmaps over the segment's rows, or NULL.
 * Output as mqvs_search (k per query, reference order, -1 padding).  With
 * MQVS_F_FIRST_STAGE the call returns the first stage only: the k best rows
 * by the approximate distance of the index's plane format (bf16 or fp8), to be re-ranked
 * by mqvs_rerank (the reference's two-stage search). */
#define MQVS_F_FIRST_STAGE 0x8u
/* Re-rank every one of the num_reorder candidates.  By default a candidate
 * whose approximate value is more than twice the query's bf16 bound past the
 * k-th best approximate value is not re-ranked: its exact value cannot reach
 * the top k, so the results are the same either way (the flag is for tests
 * and measurements). */
#define MQVS_F_RERANK_ALL 0x200u
int mqvs_index_search(mqvs_index_t idx, const float *queries, int32_t nq, int32_t k, const char *params,
                      const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                      uint32_t flags, mqvs_stream_t stream);
/* mqvs_index_search for the index of a row-range shard of a part, with the
 * cosine chunk-ordinal base given (as mqvs_search_ex: the number of granule
 * chunks before the shard's first row that the reference searches).  The
 * exact re-rank takes each row's query variant by base + the chunk's ordinal
 * within the shard.  chunk_ord_base < 0: row_offset / granule_rows, which is
 * mqvs_index_search; above INT32_MAX: MQVS_ERR_BAD_ARGUMENTS.  Only cosine
 * results depend on it, and a MQVS_F_FIRST_STAGE search ignores it. */
int mqvs_index_search_ex(mqvs_index_t idx, const float *queries, int32_t nq, int32_t k, const char *params,
                         const uint8_t *filter, const uint8_t *row_exists, int64_t chunk_ord_base,
                         int64_t *out_ids, float *out_dist, uint32_t flags, mqvs_stream_t stream);
/* Introspection of the coarse step (no reference counterpart: the MSTG
 * library's quantizer is not exposed through VectorIndex; these let a caller
 * or a test check the probes against its own exact top-nprobe):
 * mqvs_index_centroids: the nlist x dim fp32 centroid table (normalised for
 *   cosine indexes) into host memory; cap = floats out holds.
 * mqvs_index_probes: for each of nq host queries the list ids the search with
 *   `params` (alpha / nprobe as mqvs_index_search) would probe, in no
 *   guaranteed order, into out_probes[nq][nprobe] (host; nprobe as
 *   mqvs_index_last_stats then reports it; nq x nlist always suffices).
 *   For nprobe <= 64 (the coarse pick) and for indexes of more than 16384
 *   lists (a FLAT search of the centroids) the lists are the exact top nprobe
 *   by the coarse metric (L2; the raw inner product for IP and cosine parts),
 *   up to fp32 rounding of near ties; otherwise they are ranked by the bf16
 *   approximate value (the centroid list pass). */
int mqvs_index_centroids(mqvs_index_t idx, float *out, int64_t cap);
int mqvs_index_probes(mqvs_index_t idx, const float *queries, int32_t nq, const char *params, int64_t *out_probes);

/* ---- binary vector index (the reference's BINARYMSTG seam, KAT 00038) ------
 * mqvs_index_build on a binary segment (mqvs_segment_create_binary) with
 * index_type "BINARYMSTG" (also accepted: "BINARYIVF"; case-insensitive, NULL
 * = BINARYMSTG on a binary segment).  A float index type on a binary segment,
 * or a binary type on a float segment, fails with MQVS_ERR_LOGICAL.  MSTG's
 * code is absent from the reference snapshot; this is the library's own
 * design: an inverted file over k-majority (Hamming k-means) lists, the codes
 * copied in list order ([npos][code words], 16-B aligned rows), a popcount
 * scan of the lists each query probes.  Binary distances are exact integers
 * (Jaccard: one fp32 division of two integers), so the scan computes the
 * final distance: there is no approximate stage, no re-rank and no tolerance.
 * Every returned distance is bit-identical to mqvs_search_binary's on the
 * same row, and a search that probes every list equals mqvs_search_binary bit
 * for bit.
 * Build params: metric_type (Hamming | Jaccard, default the segment's; other
 * metrics MQVS_ERR_NOT_IMPLEMENTED), alpha, nlist, kmeans_iters, sample --
 * defaults and ranges as above -- and
 *   assign       valu | mfma (default valu): the kernel of the assignment
 *                passes below, row-per-lane popcounts or the i8 MFMA; the
 *                index is the same bit for bit; any other value fails with
 *                MQVS_ERR_BAD_ARGUMENTS (the float build refuses the key)
 * The list count is never chosen from the data.
 * Parts of 2^31 or more rows are MQVS_ERR_NOT_IMPLEMENTED.  The build is
 * integer arithmetic only, hence deterministic.  The coarse metric is Hamming
 * for both metrics (Jaccard parts are partitioned by Hamming, scanned with
 * Jaccard):
 *   sample       rows floor(i n / S), i < S; initial centroids are sample rows
 *                floor(c S / L), c < L
 *   iteration    each sample row goes to the centroid at the smallest Hamming
 *                distance (ties: the lowest list id); each centroid bit is
 *                then set iff 2 ones > members (majority, tie -> 0); a list
 *                with no members keeps its centroid
 *   assignment   every row to its nearest centroid by the same rule (distance
 *                == dim_bits included); lists hold their rows in ascending
 *                order
 * mqvs_index_info: dim = dim_bits, npos = rows (no padding positions),
 * hbm_bytes counts the list-ordered code copy.  mqvs_index_free,
 * mqvs_index_set_row_ids_map and mqvs_cache_put / acquire work as for float
 * indexes.
 *
 * mqvs_index_search_binary: queries are nq x dim_bits / 8 bytes.  Params:
 *   alpha, nprobe   as mqvs_index_search (nprobe <= min(nlist, 4096); nprobe ==
 *                   nlist probes every list with no ranking; the default
 *                   searches a part of up to 4 lists exhaustively)
 *   metric          Hamming | Jaccard (default the index's; either may be
 *                   searched, as mqvs_search_binary allows)
 *   num_reorder     accepted and ignored (the scan is exact)
 * The nprobe nearest centroids by (Hamming, list id) are probed.  Output
 * exactly as mqvs_search_binary: ascending by (distance, row), Hamming as
 * float counts, rows at Hamming distance == dim_bits never returned, -1 /
 * FLT_MAX padding, row_offset applied; a registered row_ids_map is applied
 * last.  MQVS_F_DEVICE_PTRS / MQVS_F_ASYNC as mqvs_index_search;
 * MQVS_F_FIRST_STAGE is accepted and returns the same exact result.
 * mqvs_index_search on a binary index, and this call on a float index, fail
 * with MQVS_ERR_LOGICAL.  mqvs_index_last_stats after it: coarse / scan /
 * select times, values = records kept by the scan (positions that pass the
 * filter and the distance rule), items, plane_bytes = code bytes of the probed
 * lists, pairs; plan_ms, rerank_ms and reranked are 0.
 * mqvs_index_centroids_binary: the nlist x dim_bits / 8 centroid bytes into
 *   host memory (cap_bytes = bytes out holds).
 * mqvs_index_probes_binary: as mqvs_index_probes for host binary queries; the
 *   lists are the exact top nprobe by (Hamming distance, list id). */
int mqvs_index_search_binary(mqvs_index_t idx, const uint8_t *queries, int32_t nq, int32_t k, const char *params,
                             const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                             uint32_t flags, mqvs_stream_t stream);
int mqvs_index_centroids_binary(mqvs_index_t idx, uint8_t *out, int64_t cap_bytes);
int mqvs_index_probes_binary(mqvs_index_t idx, const uint8_t *queries, int32_t nq, const char *params,
                             int64_t *out_probes);

/* ---- index persistence: save a built index, load it without a build ---------
 * The reference keeps index files in the part directory and loads them on a
 * cache miss (VIWithColumnInPart::serialize / ::load, VIWithDataPart.cpp:578-764;
 * VICacheManager).  A built index is determined by the segment's resident rows
 * plus five things -- the centroid table, each row's list, nlist, alpha, np95
 * -- and only those are saved: about 4 n + 4 nlist dim bytes.  The bf16 plane
 * and every other derived array is rebuilt by the load, which runs no k-means
 * and no search of rows against centroids.
 *
 * The blob is one ClickHouse CompressedWriteBuffer stream, the framing
 * mqvs_segment_create_from_column reads.  Each block:
 *   bytes 0-15   CityHash128 v1.0.2 of bytes 16 .. 24 + payload (low word first)
 *   byte  16     method: 0x02 NONE (what mqvs_index_save writes) or 0x82 LZ4
 *   bytes 17-20  UInt32 compressed size = payload bytes + 9
 *   bytes 21-24  UInt32 decompressed size
 *   bytes 25-    payload
 * mqvs_index_save writes NONE blocks of at most 1 MiB of payload;
 * mqvs_index_load reads any chain the column ingest reads, LZ4 included, so
 * the file may be re-compressed.  The decompressed content, little-endian:
 *   bytes 0-7    magic "MQVSIDX\0"
 *   bytes 8-11   UInt32 format version (MQVS_INDEX_BLOB_VERSION = 1)
 *   bytes 12-15  UInt32 kind: 0 float IVF, 1 binary IVF (MQVS_INDEX_KIND_*)
 *   bytes 16-19  UInt32 metric (mqvs_metric: the index's search metric)
 *   bytes 20-23  UInt32 dimension: dim for float, dim_bits for binary
 *   bytes 24-31  UInt64 n, the segment's rows
 *   bytes 32-39  UInt64 nlist
 *   bytes 40-43  alpha, the default search alpha, as fp32 bits
 *   bytes 44-47  UInt32 np95 (0: not measured; see mqvs_index_build)
 *   bytes 48-55  UInt64 fingerprint of the segment's resident rows (below)
 *   bytes 56-59  UInt32 list plane format (MQVS_INDEX_PLANE_*: 0 bf16, 1 fp8;
 *                zero on a binary index).  The load rebuilds the plane in this
 *                format; any other value is a malformed header.
 *   bytes 60-63  reserved, zero
 *   bytes 64-    the centroid table: nlist x dim fp32 as mqvs_index_centroids
 *                returns it (float), nlist x dim_bits / 8 bytes as
 *                mqvs_index_centroids_binary returns it (binary)
 *   then         the assignment: n Int32, each row's list id, or -1 for a row
 *                in no list (an empty array; float only).  A row the build
 *                forced into list 0 is stored as 0.
 * Nothing in it depends on the kernels' layouts (list padding, plane tiling).
 * Not saved: the row-ids map of a decoupled part (the reference keeps it in
 * the part's own files: register it again with mqvs_index_set_row_ids_map
 * after the load), the list plane (bf16 or fp8), any derived state.
 *
 * Fingerprint: S = min(n, 1024) rows, row floor(i n / S) for i < S, back to
 * back -- a float row as its dim fp32 values as resident (normalised on a
 * cosine segment), a binary row as its dim_bits / 8 bytes -- taken as the
 * payload of one method-NONE block; the fingerprint is the low 64 bits of the
 * checksum that block would carry (CityHash128 over its 9 header bytes +
 * payload).  It is computed on the device from the resident rows, in HBM or
 * in host memory (mqvs_segment_set_rows_host).
 *
 * mqvs_index_save_size: the exact size of the blob.  mqvs_index_save: the blob
 *   into the host buffer out[cap]; cap too small -> MQVS_ERR_BAD_ARGUMENTS.
 * mqvs_index_load: the index of `blob` over `seg`, as mqvs_index_build returns
 *   it: mqvs_index_info reports the built index's nlist, npos, max_list,
 *   rows_indexed, metric, dim and hbm_bytes (build_ms: the load's device
 *   time), and searches return the built index's bits.  Every check happens
 *   before any blob content is used:
 *     truncated or malformed block chain, bad magic or header field, a
 *     decompressed size other than the header implies, an assignment value
 *     outside [-1, nlist), a binary assignment of -1   MQVS_ERR_ILLEGAL_COLUMN
 *     a block checksum mismatch                         MQVS_ERR_CHECKSUM
 *     unknown format version                            MQVS_ERR_NOT_IMPLEMENTED
 *     float blob on a binary segment or the reverse; n, dimension or cosine /
 *     non-cosine family other than the segment's; fingerprint mismatch
 *                                                       MQVS_ERR_LOGICAL
 *     dimension over the list scan's limit              MQVS_ERR_BAD_ARGUMENTS
 * mqvs_index_blob_info: host only, no device call: the header fields of a
 *   blob whose first block is stored with method NONE; an LZ4 first block ->
 *   MQVS_ERR_NOT_IMPLEMENTED.  For system tables and tooling.
 * mqvs_index_lists: introspection, as mqvs_index_centroids: list_off[nlist + 1]
 *   and the part row of every position (-1 = padding) in position order. */
#define MQVS_INDEX_BLOB_VERSION 1
#define MQVS_INDEX_BLOB_HEADER_BYTES 64
#define MQVS_INDEX_KIND_FLOAT_IVF 0
#define MQVS_INDEX_KIND_BINARY_IVF 1
typedef struct {
    uint32_t version;
    uint32_t kind;         /* MQVS_INDEX_KIND_* */
    int32_t metric;
    int32_t dim;           /* dim, or dim_bits for binary */
    int64_t n;
    int64_t nlist;
    float alpha;
    int32_t np95;
    uint64_t fingerprint;
    uint64_t content_bytes; /* decompressed size the header implies */
} mqvs_index_blob_info_t;
int mqvs_index_save_size(mqvs_index_t idx, size_t *bytes);
int mqvs_index_save(mqvs_index_t idx, uint8_t *out, size_t cap, size_t *written);
int mqvs_index_load(mqvs_segment_t seg, const uint8_t *blob, size_t bytes, mqvs_index_t *out);
int mqvs_index_blob_info(const uint8_t *blob, size_t bytes, mqvs_index_blob_info_t *out);
int mqvs_index_lists(mqvs_index_t idx, int64_t *list_off, int64_t cap_off, int32_t *rows, int64_t cap_rows);

/* Decoupled parts: a part merged from several source parts whose index still
 * serves the source part's rows (the reference's VIWithMeta row_ids_map /
 * inverted maps, VICacheObject.h:50-64).
 * mqvs_index_set_row_ids_map: register the source part's row -> decoupled
 *   part row map (UInt64 per source row, len >= the indexed rows); every later
 *   mqvs_index_search on this index returns decoupled-part row ids
 *   (VIWithColumnInPart::transferToNewRowIds, VIWithDataPart.cpp:56-67, applied
 *   at :938-943).  NULL / len 0 clears it.  The map lives in HBM with the index.
 * mqvs_decoupled_filter: getRealBitmap (VIUtils.cpp:479-497) -- a PREWHERE
 *   bitmap over the decoupled part's new_rows rows -> the bitmap over this
 *   source part's old_rows rows: old bit inverted_row_ids_map[i] is set for
 *   every set bit i whose inverted_row_sources_map[i] == own_id.  With no
 *   inverted map (len 0) the filter is returned as it is.  MQVS_F_DEVICE_PTRS:
 *   all pointers on the device. */
int mqvs_index_set_row_ids_map(mqvs_index_t idx, const uint64_t *row_ids_map, int64_t len, uint32_t flags);
int mqvs_decoupled_filter(const uint8_t *new_filter, int64_t new_rows, const uint64_t *inverted_row_ids_map,
                          const uint8_t *inverted_row_sources_map, int64_t inverted_len, uint32_t own_id,
                          uint8_t *old_filter, int64_t old_rows, uint32_t flags, mqvs_stream_t stream);

/* Stats of the calling thread's last mqvs_index_search (times only with
 * mqvs_set_timing(1)). */
typedef struct {
    double coarse_ms;     /* nearest lists per query (FLAT search over the centroids) */
    double plan_ms;       /* grouping (query, list) pairs into work items */
    double scan_ms;       /* bf16 MFMA scan of the probed lists */
    double select_ms;     /* num_reorder best approximate values per query */
    double rerank_ms;     /* exact fp32 re-rank + top-k */
    double total_ms;
    int64_t values;       /* approximate values computed (query x probed position) */
    int64_t items;        /* scan work items (list x 16-query group) */
    int64_t plane_bytes;  /* list plane bytes streamed by the scan (2 per element for bf16, 1 for fp8) */
    int64_t pairs;        /* (query, list) pairs */
    int32_t nq, k, nprobe, num_reorder;
    int64_t reranked;     /* candidates re-ranked exactly (sum over queries, <= nq x num_reorder): the bf16
                             bound prunes those that cannot reach the top k (MQVS_F_RERANK_ALL: none) */
    int32_t pick_overflow;/* queries whose coarse pick found more near-tie centroid groups than its
                             working set holds and scored them in batches (the probes stay exact) */
    int32_t reserved;
} mqvs_index_search_stats;
int mqvs_index_last_stats(mqvs_index_search_stats *out);

/* ---- device-resident cache of parts (VICacheManager, VICacheManager.h:82-114)
 * An LRU of segments (+ an optional index over each) keyed by the caller's
 * CacheKey string, weighed by HBM bytes against max_bytes.
 *   put      takes ownership of seg / idx (the index must be over seg); evicts
 *            least-recently-used unheld entries to make room; a key already
 *            present is replaced (putting the same pair under its own key
 *            again only refreshes it).  MQVS_ERR_MEMORY_LIMIT when the budget
 *            cannot hold it, MQVS_ERR_BAD_ARGUMENTS for an index over another
 *            segment or a handle already cached under another key (ownership
 *            then stays with the caller).
 *   acquire  *seg = NULL on a miss; on a hit the entry is held (never evicted)
 *            and becomes most recently used; the handles stay owned by the
 *            cache.  Every hit is paired with release(key, seg).
 *   remove   forceExpire: freed now, or at the last release if held.
 * Thread-safe (one mutex; searches on acquired handles run lock-free). */
typedef struct mqvs_cache *mqvs_cache_t;
typedef struct {
    int64_t items;        /* entries in the LRU */
    size_t bytes;         /* their HBM bytes */
    size_t max_bytes;
    int64_t hits, misses, evictions;
    int64_t pinned;       /* entries held now */
    int64_t expired_held; /* removed / replaced entries still held */
} mqvs_cache_stats_t;
int mqvs_cache_create(size_t max_bytes, mqvs_cache_t *out);
int mqvs_cache_free(mqvs_cache_t cache);
int mqvs_cache_put(mqvs_cache_t cache, const char *key, mqvs_segment_t seg, mqvs_index_t idx);
int mqvs_cache_acquire(mqvs_cache_t cache, const char *key, mqvs_segment_t *seg, mqvs_index_t *idx);
int mqvs_cache_release(mqvs_cache_t cache, const char *key, mqvs_segment_t seg);
int mqvs_cache_remove(mqvs_cache_t cache, const char *key);
int mqvs_cache_stats(mqvs_cache_t cache, mqvs_cache_stats_t *out);

/* ---- observability -------------------------------------------------------
 * Stats of the calling thread's last mqvs_search: per-launch kernel times
 * (ms, HIP events on the search stream; only with mqvs_set_timing(1)), rows
 * scanned by each launch and which path ran. */
typedef struct {
    double probe_ms;        /* probe scan kernel */
    double probe_select_ms; /* radix select over the probe */
    double main_ms;         /* main scan kernels (rows [probe_rows, n), all segments) */
    double refine_ms;       /* threshold refinements between main-scan segments */
    double final_ms;        /* final select (or exact re-rank + select) kernel */
    double total_ms;        /* first to last event of the search */
    int64_t rows_scanned;
    int64_t probe_rows;
    int64_t main_rows;
    int32_t nq;
    int32_t k;
    int32_t path;           /* 0 = VALU direct formula (nq < 20), 1 = fp32 MFMA,
                               2 = bf16 MFMA pre-filter + exact fp32 re-rank,
                               3 = binary popcount scan, 4 = binary i8 MFMA
                               scan (mqvs_set_binary_batch) */
    int32_t rescans;        /* candidate-overflow re-scans / fallbacks */
    int32_t segments;       /* main-scan segments (threshold refinements + 1) */
    int32_t gather;         /* 1: selective PREWHERE, the scan walked the gather list
                               of selected rows (rows_scanned = list entries) */
    int32_t prefilter;      /* path 2: pre-filter split (2 = bf16 hi) */
    int32_t batch_kernel;   /* path 2: 1 when the main scan ran the one-wave-per-SIMD batch
                               kernel (nq > 128, contiguous rows), else 0 */
    int64_t survivors_total;/* path 2: rows re-ranked exactly (sum over queries) */
    int32_t survivors_max;  /* path 2: most rows re-ranked for one query */
    int32_t candidates_max; /* path 2: longest candidate list before the final bound */
} mqvs_search_stats;
int mqvs_last_search_stats(mqvs_search_stats *out);
/* Enable per-search HIP-event timing (off by default: one extra event pair). */
int mqvs_set_timing(int enabled);
/* Batch (nq >= 20) scan: 0 = bf16 MFMA pre-filter with a rigorous error bound
 * and exact fp32 re-rank of the survivors (default; falls back to 1 when the
 * bound admits too many rows), 1 = fp32 MFMA over every row.  Both return the
 * same bits. */
int mqvs_set_batch_mode(int mode);
/* Selective PREWHERE scans: 0 = always scan every row and mask, 1 = scan only
 * the selected rows (a device-built gather list) when few enough pass the
 * filter (default: <= 60% when the bf16 pre-filter serves the batch, <= 30%
 * for the exact small-batch kernel), 2 = always gather.  All return the same
 * bits. */
int mqvs_set_gather_mode(int mode);
/* Pre-filter planes built by segments created AFTER the call: 2 = bf16 hi
 * plane, one bf16 MFMA product bounded by measured residual norms (default;
 * 2 B per element), 0 = no planes (batches run the exact fp32 MFMA path over
 * every row).  Other values (rounds 1-2 also had 3 and 6) are
 * MQVS_ERR_BAD_ARGUMENTS.  Both return the same bits. */
int mqvs_set_prefilter(int split);
/* Device scratch that one call may allocate for large-k sorts and candidate
 * lists (default 1 GiB per buffer, at least 1 MiB): calls whose buffers would
 * exceed it run in query sub-batches, which keep the whole call's distance
 * formula (faiss's nx >= 20 branch) and return the same bits.  Returns the
 * previous value; 0 leaves it unchanged. */
size_t mqvs_set_scratch_budget(size_t bytes);
/* Process-wide cap on the device memory of all threads' search workspaces
 * (each calling thread keeps one per device: query variants, candidate lists,
 * sort scratch -- about 1 GB at nq 1000).  The reference admits 2 x physical
 * cores concurrent scans (MergeTreeVSManager.cpp:972-975); here a workspace
 * growth that would pass the cap first frees idle threads' workspaces, then
 * waits until running searches finish and give theirs back (a search that
 * ends while others wait frees its workspace).  Only when every running
 * search is waiting does one go over the cap (counted in over_budget) instead
 * of deadlocking.  Default: a quarter of the device memory.  Returns the
 * previous value; 0 leaves it unchanged.  Index searches (mqvs_index_search,
 * mqvs_decoupled_filter) pass the same gate: their scratch is counted in, and
 * trimmed with, the calling thread's workspace.  (Segments, indexes and
 * communicators are not counted.) */
size_t mqvs_set_workspace_budget(size_t bytes);
typedef struct {
    size_t budget;       /* the cap */
    size_t held;         /* device bytes of all workspaces now */
    size_t peak;         /* most held at once (since the last reset) */
    int64_t waits;       /* growths that waited for memory */
    int64_t trims;       /* workspaces freed for others */
    int64_t over_budget; /* growths let over the cap (every running search waiting) */
    int32_t active;      /* threads inside a search now */
    int32_t workspaces;  /* workspaces registered (threads x devices) */
} mqvs_workspace_stats_t;
/* reset_peak: restart peak (at held) and the counters after reading */
int mqvs_workspace_stats(mqvs_workspace_stats_t *out, int32_t reset_peak);
/* Achievable HBM read rate of this device (a bench utility: the measured
 * denominator of the scan's HBM fraction).  A STREAM-like read
 * sweep -- every lane loads 16 B, 4 loads in flight, grid-stride, 8
 * workgroups of 256 per CU -- over a fresh device buffer of `bytes` (>= 1 MiB;
 * >= 4 GiB defeats the 256 MiB Infinity Cache), best of `reps` timed passes
 * after one warm-up: *gbs = bytes / best time (1e9 B/s), *best_ms (optional). */
int mqvs_measure_read_bandwidth(size_t bytes, int32_t reps, double *gbs, double *best_ms);
/* How a calling thread waits for its GPU work (every synchronous call ends
 * with a wait; a selective PREWHERE search also waits for its selected-row
 * count).  The reference runs up to 2 x physical cores scans at once
 * (ScanThreadLimiter.h:25-58, MergeTreeVSManager.cpp:974-975): a thread that
 * spins for the length of its search holds a host core meanwhile.
 *   MQVS_WAIT_RUNTIME  hipStreamSynchronize (the HIP runtime's own policy;
 *                      on ROCm it spins, also with BlockingSync events)
 *   MQVS_WAIT_HYBRID   poll for up to spin_us, then sleep: most of the time
 *                      this thread's recent waits took, then short
 *                      sleep-polls (default, 50 us)
 *   MQVS_WAIT_BLOCK    the same without the first poll
 * Results are identical in every mode.  Returns the previous mode;
 * spin_us < 0 leaves the poll budget unchanged; other modes are
 * MQVS_ERR_BAD_ARGUMENTS (returned as a negative value: -4). */
#define MQVS_WAIT_RUNTIME 0
#define MQVS_WAIT_HYBRID 1
#define MQVS_WAIT_BLOCK 2
int mqvs_set_wait_mode(int mode, int spin_us);
/* Fault drill for a caller's host fallback (on a device error the
 * host runs its CPU path; include/mqvs_vector_index.hpp takes the fallback as
 * a callable): the next `calls` search entry points made by THIS thread --
 * mqvs_search, mqvs_search_ex, mqvs_knn_raw, mqvs_search_binary,
 * mqvs_knn_binary_raw, mqvs_index_search -- return `status` (MQVS_ERR_DEVICE
 * or MQVS_ERR_MEMORY_LIMIT) without touching the device or the outputs.
 * calls = 0 disarms.  Other statuses are MQVS_ERR_BAD_ARGUMENTS.
 * status | MQVS_FAULT_MID_CALL: the fault fires inside a filtered mqvs_search
 * instead, right after its selected-row count kernel is queued (a device
 * failure after launches; the next call must not see that call's work). */
#define MQVS_FAULT_MID_CALL 0x100
int mqvs_inject_fault(int32_t status, int32_t calls);

#ifdef __cplusplus
}
#endif
#endif /* MQVS_H */
