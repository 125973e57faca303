// flat_kernels.h -- the interface of the FLAT path's kernels (mqvs_search and
// what is built on it: the binary search, the part groups, the re-rank of an
// index search, segment preparation and column ingest).
//
// A search is a chain of launches over one ScanParams block: the query prep
// (cosine: the variant chain), a PROBE scan of the part's first rows into a
// dense matrix, the probe select (a threshold per query and the first
// candidates), APPEND scans of the rest under that threshold, and the final
// select.  Batches (nq >= 20) scan a bf16 plane first and re-rank the
// survivors in fp32.  Every scan kernel reads the same block, so the helpers
// that interpret it (tile_range, chunk_ordinal, variant_of, row_valid) live
// here with it.
//
// Where the kernels and their launchers live:
//   kernels_scan.hip     k_scan_small (VALU), k_scan_mfma, k_scan_group, k_scan_group_mfma
//   kernels_select.hip   k_probe_select, k_final_select, k_merge_shards, k_select_group, k_refine
//   kernels_bf16.hip     k_to_bf16, k_max_norm, k_query_bound, the approximate probe select, k_rerank_select
//   kernels_hi.hip       k_to_hi, k_scan_hi_* (the bf16 pre-filter scans)
//   kernels_p4.hip       k_scan_p4* (the batch scan at one wave per SIMD), k_ord_planes
//   kernels_rerank.hip   k_exact_rerank, k_rerank_ids
//   kernels_binary.hip   k_scan_binary*, k_scan_group_binary, k_hamming_to_int
//   kernels_binary_mfma.hip  k_bin_expand, k_scan_binary_mfma, k_bivf_assign_mfma (the i8 MFMA route)
//   kernels_qprep.hip    k_query_prep, k_query_prep_lds
//   kernels_filter.hip   the PREWHERE gather list, chunk ordinals, the decoupled-part filter
//   kernels_segprep.hip  k_row_norms, k_normalize_rows, k_generate, k_pack
//   kernels_ingest.hip   the column files' block table, the array sizes scan, k_array_rows
//   kernels_lz4.hip      k_decode_blocks (its sequence grammar: lz4_token.h)
//   kernels_cityhash.hip k_block_checksum
//   kernels_util.hip     k_fill2, k_words_to_host, k_async_flags, k_map_ids, the HBM read sweep
// Included by those files (some through select_common.h or scan_emit.h), by
// index_kernels.h and by workspace.h; the host side the entry points share is
// search_host.h.
#pragma once

#include <type_traits>

#include "cand_list.h"  // Cand, the candidate list's contract and its append / read functions
#include "mqvs_internal.h"

namespace mqvs {

// ---------------------------------------------------------------------------
// Ordering keys.  key32(raw) is a monotone encoding of the primary sort key
// (smaller = better) and 0xFFFFFFFF for rows the reference never returns:
//   L2:     d < FLT_MAX (faiss neutral FLT_MAX is strict, NaN never enters)
//   IP:     ip > FLT_MIN (searchWrapper's FLT_MIN init, MergeTreeVSManager.cpp:1033,1661)
//   Cosine: ip > -FLT_MAX and 1 - ip < FLT_MAX; primary key 1 - ip
__host__ __device__ inline uint32_t ord_asc(float f) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__host__ __device__ inline float cos_dist(float ip) {
    // 1 - ip exactly as VIWithDataPart.h:376 computes it (one fp32 subtraction)
    return 1.0f - ip;
}

template <int METRIC>
__host__ __device__ inline uint32_t key32(float raw) {
    const float FLTMAX = 3.40282347e+38f;
    const float FLTMIN = 1.17549435e-38f;
    if (METRIC == MQVS_METRIC_L2) {
        if (!(raw < FLTMAX)) return 0xFFFFFFFFu;
        return ord_asc(raw);
    } else if (METRIC == MQVS_METRIC_IP) {
        if (!(raw > FLTMIN)) return 0xFFFFFFFFu;
        return ~ord_asc(raw);  // descending ip
    } else if (METRIC == kMetricIpRaw) {
        if (!(raw > -FLTMAX)) return 0xFFFFFFFFu;
        return ~ord_asc(raw);
    } else {
        if (!(raw > -FLTMAX)) return 0xFFFFFFFFu;
        const float d = cos_dist(raw);
        if (!(d < FLTMAX)) return 0xFFFFFFFFu;
        return ord_asc(d);
    }
}

__host__ __device__ inline uint32_t key32_rt(int metric, float raw) {
    return metric == MQVS_METRIC_L2       ? key32<MQVS_METRIC_L2>(raw)
           : metric == MQVS_METRIC_IP     ? key32<MQVS_METRIC_IP>(raw)
           : metric == MQVS_METRIC_COSINE ? key32<MQVS_METRIC_COSINE>(raw)
                                          : key32<kMetricIpRaw>(raw);
}

// bf16 bits of x, round to nearest even (NaN stays NaN)
__host__ __device__ inline uint16_t f32_to_bf16_rn(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFF) ? 0x40 : 0));
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

__device__ inline bool bit_test(const uint8_t *bm, int64_t i) {
    return (bm[i >> 3] >> (i & 7)) & 1;
}

// ---------------------------------------------------------------------------
// Scan parameters shared by the VALU and MFMA scan kernels.
struct ScanParams {
    const float *rows;      // segment rows (normalised for cosine)
    const float *row_norms; // |y|^2 per row (L2 BLAS branch), may be null
    int64_t n;              // segment rows
    int d;
    int nq;
    const float *qvars;     // [nq][maxv][d] query variants
    const float *qnorms;    // [nq] |q|^2 (L2 BLAS branch)
    const int *qmu;         // [nq] cosine variant cycle start
    const int *qlam;        // [nq] cosine variant cycle length
    int maxv;
    int64_t chunk_rows;     // granule rows (chunking for cosine variants)
    const int *chunk_ord;   // [nchunks] ordinal, -1 = chunk never searched; null = identity
    int ord_base;           // ordinal of the segment's first chunk (row-range shards)
    const uint8_t *filter;  // PREWHERE bitmap or null
    const uint8_t *exists;  // LWD bitmap or null
    const uint8_t *nonempty;// nonempty bitmap or null (only consulted with a filter)
    int64_t row_begin, row_end;  // scan range [row_begin, row_end)
    int64_t tiles;          // number of row tiles in the range
    int64_t tiles_per_chunk;// tiles per chunk (chunk-aligned tiling) or 0 = contiguous
    int64_t tile_rows;
    // PROBE output: dense raw values [nq][probe_ld], column = row - row_begin
    float *probe;
    int64_t probe_ld;
    // APPEND output
    const uint32_t *tau;    // [nq] key threshold (inclusive)
    int *cand_count;        // [nq]
    Cand *cand;             // [nq][cand_cap]
    int cand_cap;
    int num_qblocks;        // MFMA: query blocks
    // bf16 pre-filter path (nq >= 20): hi bf16 planes, row stride dpad
    const uint16_t *rows_hi;  // row-blocked [n/16][dpad/32][16][32] (launch_to_hi)
    const uint16_t *q_hi;     // query variants, same layout, vector v q_vpad + j
    int64_t dpad;
    int64_t q_vpad;           // nq rounded up to 16 (query planes)
    // cosine ordinal planes (kernels_p4.hip): plane pl holds every query's
    // variant for chunk ordinals of class pl; desc = {m0, lam, ok}
    const uint16_t *q_ord;
    const int *q_ord_desc;
    int split;                // pre-filter planes of the scan: kHiSplit
    const float *thr;         // [nq] APPEND threshold on the approximate raw value
    // gather mode (selective PREWHERE): the scan walks positions of this list
    // of selected rows instead of rows; each chunk's rows are padded with -1 to
    // whole 256-entry tiles, so a tile never spans two chunks.  Probe columns
    // are list positions; candidates store rows.
    const int32_t *row_list;  // null = contiguous rows
    // binary scan (kernels_binary.hip)
    const uint32_t *codes;    // [n][code_words]
    const uint32_t *qcodes;   // [nq][code_words]
    int code_words;
    int nbits;                // d: Hamming distances == nbits are never returned
    int tau_strict;           // APPEND takes key < tau (segments after the probe) instead of <=
    unsigned long long *dbg;  // diagnostic builds only (stage timing stamps)
    void *p4_queue;           // batch scan (kernels_p4.hip): per-wave candidate queues, p4_queue_bytes()
    float *p4_gmax;           // batch PROBE (kernels_p4.hip): [nq][p4_gld] best approximate value per
                              // (query, 128-row half tile), as a raw metric value; NaN = no row
    int64_t p4_gld;
    int blas_nq;              // batch size that selects faiss's distance formula (0: nq); a query
                              // sub-batch of a larger call keeps the call's formula
};

// faiss's formula branch (distance_compute_blas_threshold) for this scan's call
__host__ __device__ inline bool blas_formula(const ScanParams &p) {
    return (p.blas_nq > 0 ? p.blas_nq : p.nq) >= kBlasThreshold;
}

// Row at scan position pos (-1 = padding entry of the gather list).
__device__ inline int64_t row_at(const ScanParams &p, int64_t pos) {
    return p.row_list ? (int64_t)p.row_list[pos] : pos;
}

// Tile -> [r0, r1) and chunk index ([r0, r1) are scan positions: rows, or
// gather-list positions).
__device__ inline void tile_range(const ScanParams &p, int64_t t, int64_t &r0, int64_t &r1,
                                  int64_t &chunk) {
    if (p.row_list) {
        // the first entry of a tile is a real row (padding only ends a chunk)
        r0 = p.row_begin + t * p.tile_rows;
        r1 = r0 + p.tile_rows;
        if (r1 > p.row_end) r1 = p.row_end;
        chunk = r0 < r1 ? (int64_t)p.row_list[r0] / p.chunk_rows : 0;
        return;
    }
    if (p.tiles_per_chunk > 0) {
        const int64_t c0 = p.row_begin / p.chunk_rows;  // row_begin is chunk-aligned
        chunk = c0 + t / p.tiles_per_chunk;
        r0 = chunk * p.chunk_rows + (t % p.tiles_per_chunk) * p.tile_rows;
        int64_t ce = (chunk + 1) * p.chunk_rows;
        r1 = r0 + p.tile_rows;
        if (r1 > ce) r1 = ce;
    } else {
        r0 = p.row_begin + t * p.tile_rows;
        r1 = r0 + p.tile_rows;
        chunk = p.chunk_rows > 0 ? r0 / p.chunk_rows : 0;
    }
    if (r1 > p.row_end) r1 = p.row_end;
}

// Ordinal of a granule chunk: how many searchWrapper calls the reference made
// on this part before it (cosine re-normalises the query on each call);
// -1 = the reference never searches this chunk.
__device__ inline int chunk_ordinal(const ScanParams &p, int64_t chunk) {
    if (!p.chunk_ord) return (int)chunk + p.ord_base;
    const int o = p.chunk_ord[chunk];
    return o < 0 ? o : o + p.ord_base;
}

__device__ inline int variant_of(const ScanParams &p, int q, int ord) {
    if (p.maxv <= 1) return 0;
    const int mu = p.qmu[q], lam = p.qlam[q];
    return ord < mu ? ord : mu + (ord - mu) % lam;
}

__device__ inline bool row_valid(const ScanParams &p, int64_t r) {
    if (p.filter) {
        if (!bit_test(p.filter, r)) return false;
        if (p.nonempty && !bit_test(p.nonempty, r)) return false;
    }
    if (p.exists && !bit_test(p.exists, r)) return false;
    return true;
}

// the dense PROBE value of a binary row (every binary scan: kernels_binary.hip,
// kernels_binary_mfma.hip): its distance from a = popcount(q ^ y) (Hamming) or
// a = popcount(q & y), b = popcount(q | y) (Jaccard); NaN when the row is not
// valid (or, Hamming, at distance nbits)
template <int METRIC>
__device__ __forceinline__ float bin_probe_value(uint32_t a, uint32_t b, bool valid_row, int nbits) {
    float raw;
    bool valid = valid_row;
    if (METRIC == MQVS_METRIC_HAMMING) {
        raw = (float)a;
        valid = valid && (int)a < nbits;
    } else {
        raw = a == 0u ? 1.0f : (float)(b - a) / (float)b;
    }
    return valid ? raw : __builtin_nanf("");
}

// The code width as a compile-time W4 = code_words / 4 (16-B slices per code)
// for the binary scans whose lanes read consecutive slices: f gets an
// integral_constant of 1, 2, 4 or 8, or of 0 for every other quotient (code
// rows are whole 16-B slices; the quotient is what the launchers always
// switched on).  Host side, here because the launchers of kernels_binary.hip
// and kernels_bivf.hip share no other header.
template <class F>
inline void with_w4(int code_words, F &&f) {
    switch (code_words / 4) {
        case 1: f(std::integral_constant<int, 1>{}); return;
        case 2: f(std::integral_constant<int, 2>{}); return;
        case 4: f(std::integral_constant<int, 4>{}); return;
        case 8: f(std::integral_constant<int, 8>{}); return;
        default: f(std::integral_constant<int, 0>{}); return;
    }
}

// ---------------------------------------------------------------------------
// Part groups (part_group.hip): one slot per part of a grouped launch.  The
// grouped scan maps workgroup tiles [tile0, next slot's tile0) to the part and
// writes its dense values into columns [col0, col0 + n) of the launch's
// [nq][ld] matrix; the grouped select reads each (slot, query) slice.  A
// table of m slots ends with a sentinel whose tile0 is the launch's tile count.
struct GroupSlot {
    union {
        const float *rows;
        const uint32_t *codes;  // binary parts: [n][code_words] (the segment's codes)
    };
    const float *row_norms;   // the segment's |y|^2 per row (batch scan, L2)
    const int *chunk_ord;     // as ScanParams::chunk_ord
    const uint8_t *nonempty;
    const uint8_t *filter;    // this call's PREWHERE bitmap of the part, or null
    const uint8_t *exists;    // this call's lightweight-delete bitmap, or null
    int64_t n, granule, row_offset;
    int64_t tile0, col0;
    int64_t tiles_per_chunk;  // chunk-aligned tiling of the part (0 = contiguous)
    int32_t part;             // position in the group (the merge's list index)
    int32_t pad;
};

// ---------------------------------------------------------------------------
// bf16 pre-filter path: the plane layout (written by kernels_hi.hip, read by
// kernels_hi.hip, kernels_p4.hip, kernels_bf16.hip and kernels_rerank.hip)
constexpr int kBfK = 64;    // bf16 planes padded to a multiple of this
// bf16 plane layout (rows_hi, q_hi, q_ord; written by launch_to_hi): vectors
// in groups of 16; a group is dpad / kPlaneSlab column slabs back to back, each
// [16 vectors][kPlaneSlab columns] with one vector's slab columns contiguous.
// Readers address k-step s (32 columns) of vector v16 of a group at
// plane_step_off(s) + plane_vec_off(v16).  kPlaneSlab = 32: a stage's piece
// of 16 vectors is 1 KiB contiguous (8 whole 128-B lines per wave
// instruction).  64 would give each vector one whole 128-B line per slab, so
// a gathered row (selective PREWHERE) would fetch none of its neighbour's
// bytes -- measured in round 4 (profiles/r04/layout/bench_slab64.json, every
// GPU test green): the 10 % configs[4] main scan 2.29 -> 1.88 ms, but the
// streaming scans read 16 half lines per instruction and slowed: nq 1 full
// scan 10.9 -> 13.9 ms (50M x 768), nq 1000 batch 12.6 -> 13.6 ms.
constexpr int kPlaneSlab = 32;
static_assert(kBfK % kPlaneSlab == 0, "dpad is a whole number of slabs");
__host__ __device__ constexpr uint32_t plane_vec_off(uint32_t v16) { return v16 * (uint32_t)(kPlaneSlab * 2); }
__host__ __device__ constexpr uint32_t plane_step_off(uint32_t s) {
    return (s / (uint32_t)(kPlaneSlab / 32)) * (16u * kPlaneSlab * 2) + (s % (uint32_t)(kPlaneSlab / 32)) * 64u;
}
constexpr int kHiSplit = 2; // bf16 hi*hi, bound from measured residual norms (kernels_hi.hip)
constexpr int kMxRec = 8;   // floats per vector in the norm records (launch_to_hi)

// ---------------------------------------------------------------------------
// kernels_scan.hip
void launch_scan_small(const ScanParams &p, int metric, bool probe, hipStream_t s);
void launch_scan_mfma(const ScanParams &p, int metric, bool probe, hipStream_t s);
// base: d, nq, qvars, qmu, qlam, maxv, blas_nq, probe (the matrix), probe_ld
// set; the per-part fields come from the slots
void launch_scan_group(const ScanParams &base, const GroupSlot *slots, int nslots, int64_t tiles, int metric,
                       hipStream_t s);
// the batch form (nq >= kBlasThreshold): k_scan_mfma's work items, tiles of
// kMfmaRows rows; base also holds qnorms and num_qblocks
void launch_scan_group_mfma(const ScanParams &base, const GroupSlot *slots, int nslots, int64_t tiles, int metric,
                            hipStream_t s);

// ---------------------------------------------------------------------------
// kernels_select.hip
void launch_probe_select(const float *probe, int64_t P, int64_t ld, int nq, int k, int metric,
                         uint32_t *tau, int *cand_count, Cand *cand, int cand_cap,
                         int64_t row_base, const int32_t *row_list, hipStream_t s);
// scratch: null, or 2 kLargeCap uint4 records per query (k > kSortCap)
void launch_final_select(const Cand *cand, const int *cand_count, int cand_cap, int nq, int k,
                         int metric, int64_t chunk_rows, int64_t id_offset, int64_t *out_ids,
                         float *out_dist, int *overflow, uint4 *scratch, hipStream_t s);
// scratch: 2 nshards k uint4 records per query when nshards k > kSortCap
// out_list (optional): [nq][k] the list each result came from, -1 in padding
void launch_merge_shards(int nshards, int nq, int k, int metric, const int64_t *in_ids,
                         const float *in_dist, int64_t *out_ids, float *out_dist, bool part_merge,
                         uint4 *scratch, hipStream_t s, int32_t *out_list = nullptr);
// per (slot, query) the k best rows of the slice in mqvs_search's order ->
// list_ids / list_dist [group parts][nq][k] at the slot's part
void launch_select_group(const float *matrix, int64_t ld, const GroupSlot *slots, int nslots, int nq, int k,
                         int metric, int64_t *list_ids, float *list_dist, int *overflow, hipStream_t s);
void launch_refine(const Cand *cin, const int *cnt_in, int cap, int nq, int k, int metric,
                   bool approx, const float *bq, uint32_t *tau, float *thr, Cand *cout, int *cnt_out,
                   hipStream_t s);

// ---------------------------------------------------------------------------
// kernels_bf16.hip
// dst_hi = bf16_rn(x), row-major [rows][dpad] (the index's list planes)
void launch_to_bf16(const float *src, int64_t rows, int d, int64_t src_stride, uint16_t *dst_hi, int64_t dpad,
                    hipStream_t s);
void launch_max_norm(const float *norms2, int64_t n, float *out_max, hipStream_t s);
// qrec [nq][maxv][kMxRec] query-variant norm records, yrec [kMxRec] segment maxima
// flags (may be null): the search's overflow word; bit 4 (as k_survivors':
// the exact path must serve the search) is set for a query whose norm is NaN
// or at least 1e18
void launch_query_bound(const ScanParams &p, int metric, const float *ynorm_max, const float *qrec,
                        const float *yrec, float *bq, int *flags, hipStream_t s);
void launch_probe_select_approx(const float *probe, int64_t P, int64_t ld, int nq, int k,
                                int metric, const float *bq, float *thr, int *cand_count,
                                Cand *cand, int cand_cap, const int32_t *row_list, hipStream_t s);
// fl / host_fl (optional): the final select's first workgroup also stores the
// 8 words fl (written by earlier kernels of the stream) into pinned host_fl --
// the search's status copy without a kernel of its own
void launch_rerank_select(const ScanParams &p, int metric, const float *bq, int k, int64_t id_offset,
                          int64_t *out_ids, float *out_dist, int *overflow, uint32_t *surv, int *scnt,
                          uint4 *recs, int lcap, int64_t rs, hipStream_t s, const int *fl = nullptr,
                          int *host_fl = nullptr);

// ---------------------------------------------------------------------------
// kernels_hi.hip
// split 2: row-blocked bf16 hi plane (16 vectors x 32
// columns contiguous; source vector v goes to plane vector
// (v % vgroup) vpad + v / vgroup) + records [|h|, |r|, -, -, -, -, |x|] per
// vector (rec) / maxima (maxrec, atomic)
void launch_to_hi(const float *src, int64_t rows, int d, int64_t src_stride, int64_t dpad, int64_t vgroup,
                  int64_t vpad, uint16_t *hi, float *rec, float *maxrec, hipStream_t s);
void launch_scan_hi(const ScanParams &p, int metric, bool probe, hipStream_t s);
bool scan_hi_small_tiles_ok(int nq, int64_t dpad);
int take_batch_kernel_flag();  // 1 when a main scan since the last call ran kernels_p4 (then cleared)

// ---------------------------------------------------------------------------
// kernels_p4.hip
// batch APPEND scan at one wave per SIMD: false when the
// scan's shape is not served (gather lists, chunk-ordinal tables, no queue)
bool launch_scan_p4(const ScanParams &p, int metric, hipStream_t s);
// the batch probe (p.p4_gmax, p.p4_gld >= 2 p.tiles): false when the rows
// cannot take the batch kernel
bool launch_scan_p4_probe(const ScanParams &p, int metric, hipStream_t s);
// the batch probe by 16-row groups: p.p4_gmax[q][16 t + r]
// = the best value of rows [16 r, 16 r + 16) of tile t (p.p4_gld >= 16
// p.tiles); false when the rows cannot take the batch kernel
bool launch_scan_p4_groups(const ScanParams &p, int metric, hipStream_t s);
// cosine ordinal planes for the batch kernel: at most pcap planes, built on
// the device from q_hi / qmu / qlam (desc[2] = 0 when the chains need more)
constexpr int kP4OrdPlanesMax = 32;
void launch_ord_planes(const uint16_t *q_hi, uint16_t *q_ord, int *desc, const int *qmu, const int *qlam, int nq,
                       int64_t vpad, int64_t dpad, int pcap, hipStream_t s);
size_t p4_queue_bytes();  // p4_queue workspace for the current device

// ---------------------------------------------------------------------------
// kernels_rerank.hip
// Bound pruning of an index re-rank: the candidates come
// sorted by their approximate value; those more than 2 B past the k-th
// approximate value cannot reach the exact top k and are not re-ranked (same
// output).  raw = null: every candidate is re-ranked.
struct RerankPrune {
    const float *raw = nullptr;           // [nq][ncand] approximate raw values in candidate order (NaN: none)
    const float *bq = nullptr;            // [nq] bound on |approx - exact| for query variant 0 (k_query_bound)
    const float *ymax = nullptr;          // device scalar: max |y| over the rows (cosine variant term)
    const float *qdelta = nullptr;        // [nq] cosine: >= max_v |x_v - x_0| (k_query_prep); null: computed here
    unsigned long long *count = nullptr;  // += candidates re-ranked (may be null)
};
void launch_rerank_ids(const ScanParams &p, int metric, const int64_t *cand, int ncand, int k,
                       int64_t id_offset, int64_t *out_ids, float *out_dist, uint4 *scratch, hipStream_t s,
                       const RerankPrune &prune = RerankPrune{});
void launch_exact_rerank(const ScanParams &p, int metric, const uint32_t *surv, const int *cnt, int64_t rs,
                         int cap, uint4 *recs, int k, int64_t id_offset, int64_t *out_ids, float *out_dist,
                         hipStream_t s, const int *fl = nullptr, int *host_fl = nullptr);

// ---------------------------------------------------------------------------
// kernels_binary.hip (binary vectors)
void launch_scan_binary(const ScanParams &p, int metric, bool probe, hipStream_t s);
// binary parts of a group: the PROBE values of k_scan_binary /
// k_scan_binary_co, tiles of kSmallRows rows; base: nq, qcodes, code_words,
// nbits, probe (the matrix), probe_ld set
void launch_scan_group_binary(const ScanParams &base, const GroupSlot *slots, int nslots, int64_t tiles, int metric,
                              hipStream_t s);
void launch_hamming_to_int(const int64_t *ids, float *dist, int64_t m, hipStream_t s);

// ---------------------------------------------------------------------------
// kernels_binary_mfma.hip (binary vectors on the i8 MFMA)
// bytes of the expanded plane of ncols codes (columns padded to 16)
inline size_t bin_plane_bytes(int64_t ncols, int code_words) {
    return (size_t)((ncols + 15) / 16 * 16) * (size_t)code_words * 32;
}
// plane[col][k] = bit k of codes[col] as a 0/1 byte, pop[col] = popcount of the
// code; both cover ncols rounded up to 16 columns (padding: zeros)
void launch_bin_expand(const uint32_t *codes, int ncols, int code_words, uint8_t *plane, uint32_t *pop,
                       hipStream_t s);
// the columns of a product in operand form (launch_bin_expand's outputs)
struct BinPlane {
    const uint8_t *plane;   // [columns rounded up to 16][code_words * 32] codes as 0/1 bytes
    const uint32_t *pop;    // [columns rounded up to 16] popcount of each code
};
// launch_scan_binary's contract on the i8 MFMA (any nq; q: p.qcodes through
// launch_bin_expand; p.tiles / p.tile_rows are not read).  The plane travels
// beside ScanParams, not in it: the block's layout is every other scan
// kernel's argument layout.
void launch_scan_binary_mfma(const ScanParams &p, const BinPlane &q, int metric, bool probe, hipStream_t s);

// ---------------------------------------------------------------------------
// kernels_qprep.hip
// maxv: variants stored per query (1 unless cosine)
// phase: 0 everything; 1 variant 0 only; 2 the rest of the chain (after 1)
void launch_query_prep(const float *q, int nq, int d, int metric, bool blas, float *qvars, int maxv,
                       float *qnorms, int *qmu, int *qlam, int *status, hipStream_t s, int phase = 0,
                       float *qdelta = nullptr);

// ---------------------------------------------------------------------------
// kernels_filter.hip
void launch_gather_count(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists, int64_t n,
                         int64_t chunk_rows, int tile, int *count, int64_t *offsets, int64_t *totals,
                         int64_t *host_totals, int64_t host_gen, int *ticket, hipStream_t s);
void launch_gather_list(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists, int64_t n,
                        int64_t chunk_rows, int tile, const int *count, const int64_t *offsets, int32_t *list, int64_t list_end,
                        hipStream_t s, const int64_t *dev_total = nullptr, int64_t round = 1);
void launch_chunk_ordinals(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists,
                           int64_t n, int64_t chunk_rows, int require_filter, int *ord,
                           hipStream_t s);
// number of granule chunks of [0, n) the reference searches (a non-empty row
// that, under a PREWHERE filter, passes it and is not deleted) -> *count
void launch_count_active_chunks(const uint8_t *filter, const uint8_t *nonempty, const uint8_t *exists, int64_t n,
                                int64_t chunk_rows, int *flags_scratch, int64_t *count, hipStream_t s);
// decoupled parts (index.hip): new-part filter -> old-part filter
// (getRealBitmap): old bit inv_ids[i] for every set new bit i < inv_len with
// inv_src[i] == own_id (inv_ids null: the filter passes through unchanged);
// old_words is zeroed first, (old_rows + 31) / 32 words.
void launch_decoupled_filter(const uint8_t *new_filter, int64_t new_rows, const uint64_t *inv_ids,
                             const uint8_t *inv_src, int64_t inv_len, uint32_t own_id, uint32_t *old_words,
                             int64_t old_rows, hipStream_t s);

// ---------------------------------------------------------------------------
// kernels_segprep.hip
void launch_normalize_rows(float *rows, int64_t n, int d, hipStream_t s);
void launch_row_norms(const float *rows, int64_t n, int d, float *norms, hipStream_t s);
void launch_generate(uint64_t seed, int mode, int64_t row0, int64_t n, int d, float *out,
                     hipStream_t s);
void launch_pack_nonempty(const uint8_t *bytes, int64_t n, uint8_t *bits, hipStream_t s);

// ---------------------------------------------------------------------------
// kernels_ingest.hip, kernels_lz4.hip (launch_decode_blocks), kernels_cityhash.hip
// (launch_block_checksum): compressed MergeTree column files -> rows; the index blob's framing
struct IngestBlock {
    int64_t src;      // payload offset in the compressed stream
    int64_t dst;      // offset in the decompressed stream
    uint32_t csize;   // payload bytes
    uint32_t usize;   // decompressed bytes
    uint32_t method;  // 0x82 LZ4, 0x02 NONE
    uint32_t pad;
};
void launch_block_table(const uint8_t *src, int64_t n, IngestBlock *tab, int64_t max_blocks, int64_t *out,
                        hipStream_t s);
void launch_decode_blocks(const uint8_t *src, int64_t src_bytes, const IngestBlock *tab, int64_t nblocks, uint8_t *dst,
                          int *status, hipStream_t s);
// CityHash128 of block i's header + payload != its stored checksum -> *status |= flag;
// hash_out (optional) receives [nblocks][2] (low, high)
void launch_block_checksum(const uint8_t *src, const IngestBlock *tab, int64_t nblocks, int flag, int *status,
                           uint64_t *hash_out, hipStream_t s);
void launch_sizes_scan(const uint64_t *sizes, int64_t n, int d, int64_t max_size, int64_t *offsets, int64_t *scratch,
                       int64_t *stats, hipStream_t s);
void launch_array_rows(const float *data, const int64_t *offsets, const uint64_t *sizes, int64_t n, int d,
                       float *rows, uint8_t *nonempty, hipStream_t s);

// ---------------------------------------------------------------------------
// kernels_util.hip
// up to two 32-bit fills (a: na words of va, b: nb words of vb) in one launch
void launch_fill2(uint32_t *a, int64_t na, uint32_t va, uint32_t *b, int64_t nb, uint32_t vb, hipStream_t s);
// a[0, na) and b[0, nb) into pinned host memory (system-scope stores; one
// launch instead of two copy kernels before the caller's stream sync)
// (pq: a's words are the sums over npq rows of pq[npq][na] instead)
void launch_words_to_host(const int64_t *a, int na, const int *b, int nb, int64_t *host_a, int *host_b,
                          hipStream_t s, const int64_t *pq = nullptr, int npq = 0);
// ASYNC calls: OR a search's device flags into the calling thread's sticky
// word (read and cleared by mqvs_async_check): bit 0 = candidate overflow
// (overflow[0] != 0), bit 1 = cosine variant chain did not repeat (status[0]
// != 0 and status_matters).  overflow / status may be null.
void launch_async_flags(const int *overflow, const int *status, int status_matters, int *sticky, hipStream_t s);
// decoupled parts (index.hip): ids[i] = map[ids[i]] for ids >= 0
// (transferToNewRowIds)
void launch_map_ids(int64_t *ids, int64_t count, const uint64_t *map, hipStream_t s);
// the HBM read sweep (the benchmark's measured denominator): best rate in GB/s
double measure_read_sweep(size_t bytes, int reps, hipStream_t s, double *best_ms);

// (the index kernels' parameter blocks and launchers, float and binary:
// index_kernels.h)

}  // namespace mqvs
