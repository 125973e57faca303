// index_kernels.h -- the interface of the index path's kernels (mqvs_index_*):
// the MSTG-type index (the reference's Search::VectorIndex behind
// VIWithColumnInPart::search, VIWithDataPart.cpp:858-957) laid out for HBM.
//
// Layout.  The part's rows are partitioned into `nlist` lists by a k-means
// coarse quantizer.  The lists are stored back to back as one bf16 plane in
// list order (each list padded to a multiple of 16 positions; blocked as
// [npos / 16][dpad / 32][16][32], 1 KiB pieces like the FLAT plane),
// with perm[pos] = segment row (-1 = padding) and pnorm[pos] = |y|^2.
//
// Search (one batch of nq queries, each probing nprobe lists):
//   k_plan_*      group the nq*nprobe (query, probe) pairs by list, cut each
//                 list's queries into 16-query work items, and give every
//                 pair its region of the candidate buffer
//   k_ivf_scan    per work item: stream the list's bf16 rows from HBM straight
//                 into MFMA A fragments (v_mfma_f32_16x16x32_bf16), the 16
//                 queries as B from LDS; approximate values to the regions
//   k_ivf_select  per query: radix-select the num_reorder best approximate
//                 values, ordered compaction, bitonic sort in LDS
// then the exact fp32 re-rank (k_rerank_ids, kernels_rerank.hip).
//
// An index built with plane=fp8 keeps the plane as e4m3fn codes at 1 B per
// element instead (k_to_fp8; k_ivf_scan_fp8 widens them to bf16 in registers);
// plan, select and re-rank are the same.
//
// Where the kernels and their launchers live:
//   kernels_ivf_plan.hip    k_plan_*, k_iota_probes
//   kernels_ivf_scan.hip    k_ivf_scan, k_ivf_scan_fp8
//   kernels_ivf_select.hip  k_ivf_select, k_ivf_select_small
//   kernels_ivf_pick.hip    k_coarse_pick (the coarse step's exact pick)
//   kernels_ivf_build.hip   k_ivf_pack, k_to_fp8, k_gather_rows, k_centroid_mean, k_grp_*
//   kernels_bivf.hip        the binary index: k_bivf_*, and k_bivf_group_* (index groups)
//   kernels_select.hip      k_bivf_group_select (the final select's body per (slot, query))
// Included by index_internal.h (the host files) and those seven files only.
#pragma once

#include "flat_kernels.h"

namespace mqvs {

// ---------------------------------------------------------------------------
// Index path (kernels_ivf_*.hip, index_build.hip, index_search.hip)
constexpr int kIvfPad = 16;  // list lengths padded to this many positions

constexpr int kIvfChunk = 512;  // default list positions per scan work item (balances long and short lists)

struct IvfParams {
    const uint16_t *plane;    // [npos][dpad] bf16 rows in list order
    const int32_t *perm;      // [npos] segment row of each position, -1 = padding
    const float *pnorm;       // [npos] |y|^2 per position
    const int64_t *list_off;  // [nlist+1] list start positions (multiples of kIvfPad)
    int nlist;
    int64_t dpad;
    int nq, nprobe;
    int qg;                   // queries per scan work item: 16 or 32 (MFMA B blocks x 16)
    int chunk;                // list positions per scan work item (multiple of 64)
    const int64_t *probes;    // [nq][nprobe] list ids (-1 = none)
    const uint16_t *q_hi;     // [nq][dpad] bf16 query (cosine: normalised)
    const float *qnorm;       // [nq] |q|^2 (L2)
    const uint8_t *filter;    // PREWHERE bitmap (rows) or null
    const uint8_t *exists;    // LWD bitmap (rows) or null
    int *lcount;              // [nlist] queries probing each list
    int *lfill;               // [nlist] scatter cursors
    int64_t *lstart;          // [nlist] first pair of each list in lq
    int *lq;                  // [nq*nprobe] pairs (q*nprobe + probe) grouped by list
    int *item_list;           // [nq*nprobe] work item -> list
    int *item_grp;            // work item -> query group within the list
    int *item_chk;            // work item -> slice of the list
    int *nitems;              // number of work items
    int64_t *qbase;           // [nq*nprobe] start of each pair's region in cand
    int64_t *qstart;          // [nq+1] start of each query's region
    Cand *cand;               // approximate values, one per (pair, list position)
    int64_t *stats;           // [4] values written, items, plane bytes, pairs
    int64_t *bsum;            // [3 * plan workgroups] per-workgroup list totals (k_plan_lists_blk)
    // pair mode (pair_stride > 0; few pairs per list): no plan -- work item
    // it is (pair it / pair_nch, slice it % pair_nch) of one query, query q's
    // region starts at q * pair_stride and holds its probes' lists back to back
    int64_t pair_stride;
    int pair_nch;
    // fp8 list plane (plane8 non-null: k_ivf_scan_fp8; `plane` unused, q_hi
    // holds the queries' scaled e4m3fn codes as bf16 values)
    const uint8_t *plane8;    // e4m3fn codes, [npos/16][dpad/64][16][64] (k_to_fp8)
    const int16_t *pscale;    // [npos] scale exponent e_p of each position
    const int16_t *qexp;      // [nq] scale exponent e_q of each query
    int esize;                // bytes per plane element: 2 (bf16) or 1 (fp8)
};

// The per-query candidate regions of a list pass, as the select reads them:
// the plan's qstart[nq + 1], or pair mode's fixed strides (regions filled by
// the probed lists' lengths; the select then also sums the stats).
struct IvfRegions {
    const int64_t *qstart = nullptr;
    int64_t stride = 0;
    int nprobe = 0, nlist = 0, chunk = 0;
    int64_t dpad = 0;
    const int64_t *probes = nullptr;
    const int64_t *list_off = nullptr;
    int64_t *stats = nullptr;  // pair mode: [nq][4] values, items, plane bytes, pairs per query
    int esize = 2;             // bytes per plane element (the stats' plane bytes)
};

// LDS of one k_ivf_scan workgroup with qg-query work items: the query tile
// (qg rows of 2 dpad + 16 B, dynamic) + 16 B of pair records per query (static)
inline int64_t ivf_scan_lds(int qg, int64_t dpad) { return (int64_t)qg * (2 * dpad + 16) + 16 * (int64_t)qg; }
// The largest of `want` (64, 32 or 16) and its smaller siblings whose tile fits
// lds_limit bytes; 0: not even 16 queries fit (no list scan at this width).
// With the 160 KiB of a gfx950 workgroup: 64 up to dpad 1216, 32 up to 2496,
// 16 up to 5056.
inline int ivf_fit_qg(int want, int64_t dpad, int64_t lds_limit) {
    for (int qg = want; qg >= 16; qg >>= 1)
        if (ivf_scan_lds(qg, dpad) <= lds_limit) return qg;
    return 0;
}
void launch_ivf_plan(const IvfParams &p, hipStream_t s);
void launch_iota_probes(int64_t *probes, int nq, int np, hipStream_t s);
void launch_ivf_plan_dense(const IvfParams &p, int64_t npos, hipStream_t s);
void launch_ivf_scan(const IvfParams &p, int metric, int grid, hipStream_t s);
// expect_len: typical per-query region length (sizes the LDS key cache)
void launch_ivf_select(const Cand *cand, const IvfRegions &rg, int nq, int R, int metric, int64_t *out_rows,
                       int64_t id_offset, float *out_approx, int64_t expect_len, hipStream_t s, uint4 *gscr = nullptr,
                       float *out_raw = nullptr);
void launch_ivf_pack(const float *rows, const float *norms, int d, const int32_t *perm, int64_t npos, int64_t dpad,
                     uint16_t *plane, float *pnorm, hipStream_t s);
// fp8 (OCP e4m3fn) quantisation of m vectors with one power-of-two scale
// each (the rule in include/mqvs.h, mqvs_index_build): vector v is row perm[v]
// of src (perm null: row v; perm[v] < 0: a padding position, zero codes).
// codes (optional): the list plane's [m/16][dpad/64][16][64] layout; hi
// (optional): the scaled codes' values as bf16, row-major [m][dpad] (queries).
// expo[v] = the scale exponent; pnorm (optional): the
// row's norms[perm[v]]; rec (optional): [m][kMxRec] records [0] |v8|, [1] |v -
// v8|, [6] |v| (v8 the de-scaled codes); maxrec (optional): their maxima over
// the vectors that are not padding, non-finite for a non-finite vector.
void launch_to_fp8(const float *src, int64_t src_ld, int d, const int32_t *perm, int64_t m, int64_t dpad,
                   uint8_t *codes, uint16_t *hi, int16_t *expo, const float *norms, float *pnorm, float *rec,
                   float *maxrec, hipStream_t s);
void launch_gather_rows(const float *src, int64_t src_ld, int d, const int64_t *idx, int64_t m, float *dst,
                        hipStream_t s);
constexpr int kCoarsePickMaxT = 64;  // core groups (and nprobe) of a coarse pick
constexpr int kCoarsePickCap = 128;  // groups a pick's working set holds (more: its batched overflow path)
// the coarse step's pick from the batch probe's 16-centroid group maxima
// (kernels_ivf_pick.hip): per query the T best groups (T <= 64) and every group
// within 2 bq[q] of the T-th (bq: the query's bf16 bound, k_query_bound;
// null = none), the exact values of their centroids (coarse metric: L2 or
// kMetricIpRaw), the nprobe best -> probes[q][0, nprobe) (-1 when fewer)
void launch_coarse_pick(const float *gmax, int64_t gld, int64_t ngroups, int T, int nprobe, int metric,
                        const float *q, int64_t qld, const float *cent, const float *cnorm, int64_t ncent, int d,
                        const float *bq, const float *qnorms, int gs_log2, int nq, int64_t *probes,
                        unsigned long long *ovf, hipStream_t s);
void launch_centroid_mean(const float *rows, int d, const int32_t *order, const int64_t *off, int nlist, float *cent,
                          hipStream_t s);
// Rows grouped by list on the device (kernels_ivf_build.hip; index_build.hip's
// finish_index).  assign[n]: list id of each row, -1 = in no list; a row whose
// nonempty bit (may be null) is clear is in no list.
// count: cnt[L] (zeroed) rows per list; *status (zeroed) |= kGrpBadRange for a
// value outside [-1, L) -- it is not counted --, kGrpNoList for a -1 when
// !allow_none.  scan: off[L + 1] (lengths rounded up to pad) and info[5] =
// npos, longest list in positions, rows in lists, rows of the longest list,
// *status.  scatter (after the host has read info: perm[npos] filled with
// -1, fill[L] zeroed) + sort: perm as a stable counting sort gives it; tmp
// (npos words) is needed when max_rows > kSortCap, and the result is in the
// returned one of perm / tmp.
constexpr int kGrpStatusBadRange = 1, kGrpStatusNoList = 2;
void launch_grp_count(const int32_t *assign, int64_t n, int64_t L, const uint8_t *nonempty, bool allow_none, int *cnt,
                      int *status, hipStream_t s);
void launch_grp_scan(const int *cnt, int64_t L, int pad, int64_t *off, int64_t *info, const int *status,
                     hipStream_t s);
void launch_grp_scatter(const int32_t *assign, int64_t n, int64_t L, const uint8_t *nonempty, const int64_t *off,
                        int *fill, int32_t *perm, hipStream_t s);
int32_t *launch_grp_sort(int32_t *perm, int32_t *tmp, const int64_t *off, const int *cnt, int64_t L, int64_t npos,
                         int64_t max_rows, hipStream_t s);
// assign[perm[pos]] = list of pos (assign[n] filled with -1 by the caller)
void launch_grp_assign_of(const int32_t *perm, const int64_t *off, int64_t L, int64_t npos, int64_t n,
                          int32_t *assign, hipStream_t s);
// a build's nearest-centroid ids (int64; null = all 0) -> canonical assignment:
// outside [0, L) -> list 0, empty array -> -1
void launch_grp_canon(const int64_t *assign, int64_t n, int64_t L, const uint8_t *nonempty, int32_t *out,
                      hipStream_t s);

// ---------------------------------------------------------------------------
// Binary index path (kernels_bivf.hip, index_build.hip, index_search_binary.hip)
struct BivfParams {
    const uint32_t *plane;    // [npos][code_words] codes in list order
    const int32_t *perm;      // [npos] part row of each position
    const int64_t *list_off;  // [nlist+1] list start positions
    int nlist;
    int code_words;
    int nbits;                // Hamming distances == nbits are never returned
    int nq, nprobe;
    int nch;                  // 256-position slices per (query, probed list): ceil(longest list / 256)
    const int64_t *probes;    // [nq][nprobe] list ids
    const uint32_t *qcodes;   // [nq][code_words]
    const uint8_t *filter;    // PREWHERE bitmap (rows) or null
    const uint8_t *exists;    // LWD bitmap (rows) or null
    Cand *cand;               // [nq][cand_cap] (distance, part row) of the kept positions
    int *cand_count;          // [nq]
    int cand_cap;
};
void launch_bivf_assign(const uint32_t *codes, int64_t n, int code_words, const uint32_t *cent, int nlist,
                        int32_t *assign, hipStream_t s);
// the same assignment on the i8 MFMA (kernels_binary_mfma.hip); cplane / cpop:
// scratch of bin_plane_bytes(nlist, code_words) bytes and nlist rounded up to
// 16 words for the expanded centroids; code_words * 32 < 2^24
void launch_bivf_assign_mfma(const uint32_t *codes, int64_t n, int code_words, const uint32_t *cent, int nlist,
                             uint8_t *cplane, uint32_t *cpop, int32_t *assign, hipStream_t s);
// counts [nlist][code_words][32] and members [nlist] must be zero
void launch_bivf_majority(const uint32_t *codes, int64_t m, int code_words, const int32_t *assign, int nlist,
                          uint32_t *counts, uint32_t *members, uint32_t *cent, hipStream_t s);
void launch_bivf_gather(const uint32_t *src, int code_words, const int32_t *idx, int64_t m, uint32_t *dst,
                        hipStream_t s);
// cdist: [nq][nlist] words of scratch; nprobe < nlist
void launch_bivf_coarse(const uint32_t *cent, int nlist, int code_words, const uint32_t *qcodes, int nq, int nprobe,
                        uint32_t *cdist, int64_t *probes, hipStream_t s);
// metric: Hamming or Jaccard; stats (optional): [4] values, items, plane bytes, pairs
void launch_bivf_scan(const BivfParams &p, int metric, int64_t *stats, hipStream_t s);

// ---------------------------------------------------------------------------
// Binary index groups (index_group.hip): one slot per fused part of a grouped
// launch chain.  A slice's table of m slots ends with a sentinel (part -1)
// whose prefix sums are the slice's totals.  cent0 / ctile0 / item0 / cand0
// restart in every slice (the centroid-distance matrix and the records are the
// slice's scratch); probe0 / count0 run over the whole call, whose probes and
// record counts stay for the stats kernel.
struct BivfGroupSlot {
    const uint32_t *bcent;        // [nlist][code_words] the part's centroids
    const uint32_t *bplane;       // [npos][code_words] codes in list order
    const int32_t *perm;          // [npos] part row of each position
    const int64_t *list_off;      // [nlist+1]
    const uint8_t *filter;        // this call's PREWHERE bitmap of the part, or null
    const uint8_t *exists;        // this call's lightweight-delete bitmap, or null
    const uint64_t *row_ids_map;  // the part's row-ids map (decoupled part), or null
    int64_t row_offset;
    int64_t cent0;                // the part's column in the [nq][sum nlist] distance matrix (ranked slots)
    int64_t ctile0;               // centroid tiles, nq * ceil(nlist / 256) per ranked slot
    int64_t probe0;               // probes, nq * nprobe per slot: probes[probe0 + q * nprobe + r]
    int64_t item0;                // scan work items, nq * nprobe * nch per slot
    int64_t cand0;                // records, nq * cap per slot: region (slot, q) at cand0 + q * cap
    int64_t count0;               // record counters, nq per slot
    int32_t nlist;
    int32_t nprobe;               // == nlist: every list in order, no ranking
    int32_t nch;                  // ceil(longest list / 256)
    int32_t cap;                  // records per (slot, query) region: every position of the probed lists
    int32_t part;                 // position in the group (the merge's list index); -1: the sentinel
    int32_t pad;
};
// cdist: the slice's [nq][ld] words (ld = the sentinel's cent0, ctiles its
// ctile0); also zeroes the slots' record counters
void launch_bivf_group_coarse(const BivfGroupSlot *slots, int nslots, int64_t ctiles, int code_words,
                              const uint32_t *qcodes, int nq, uint32_t *cdist, int64_t ld, int64_t *probes, int *count,
                              hipStream_t s);
// base: code_words, nbits, nq, qcodes, probes, cand set; the per-part fields come from the slots
void launch_bivf_group_scan(const BivfParams &base, const BivfGroupSlot *slots, int nslots, int64_t items, int *count,
                            int metric, hipStream_t s);
// kernels_select.hip: per (slot, query) the k best records of the region by
// (distance, part row) -> list_ids / list_dist [group parts][nq][k] at the slot's part
void launch_bivf_group_select(const Cand *cand, const int *count, const BivfGroupSlot *slots, int nslots, int nq,
                              int k, int64_t *list_ids, float *list_dist, int *overflow, hipStream_t s);
// over all nentries table entries of the call (sentinels included, skipped)
void launch_bivf_group_map(const BivfGroupSlot *slots, int nentries, int64_t per_part, int64_t *list_ids,
                           hipStream_t s);
// stats[4] (zeroed) += values, items, plane bytes, pairs of every slot
void launch_bivf_group_stats(const BivfGroupSlot *slots, int nentries, int nq, int code_words, const int64_t *probes,
                             const int *count, int64_t *stats, hipStream_t s);

}  // namespace mqvs
