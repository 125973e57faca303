// part_group.hip -- many small resident parts searched in one fused call
// (mqvs_part_group_*, include/mqvs.h).
//
// The fused route is the FLAT search's exact small-batch path with a batch
// dimension over parts:
//   1. query prep        once per call (the cosine variant chain belongs to
//                        the query; the table covers the part with the most
//                        chunk ordinals)
//   2. grouped scan      k_scan_group: k_scan_small's PROBE tiles of every
//                        fused part -> dense raw values [nq][sum n_p]
//   3. grouped select    k_select_group: k_final_select's body per (part,
//                        query) over the part's slice -> per-part top-k lists
//   4. merge             k_merge_shards (part merge) with the list index out
// The batch route (nq >= 20, opted in by mqvs_set_part_group_batch) is the
// same chain on the exact fp32 BLAS-branch scan: the query prep also produces
// |q|^2 for L2, step 2 is k_scan_group_mfma (k_scan_mfma's PROBE work items,
// 128-row tiles), steps 3 and 4 are unchanged.
// Parts the fused route does not take run mqvs_search's own path on the same
// stream into their list of the same merge.  Nothing here depends on what a
// kernel found: the call has one host wait, after the merge.
//
// A group of binary (FixedString) segments is searched by
// mqvs_part_group_search_binary: the query codes uploaded once, steps 2 - 4
// with k_scan_group_binary (the PROBE values of mqvs_search_binary's popcount
// scans) and the L2 order, at any nq; the per-part route is search_binary.
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "group_call.h"

struct mqvs_part_group {
    std::vector<mqvs_segment *> segs;
    int device = 0;
    int d = 0;  // binary: dim_bits
    bool cos = false;
    bool binary = false;  // FixedString segments, all of one width
    int code_bytes = 0, code_words = 0;
    int64_t rows = 0;
};

namespace mqvs {

constexpr int64_t kGroupRowsMax = (int64_t)1 << 24;  // a part's slice is indexed by int
// the fused route's row limit (mqvs_set_part_group_rows).  Measured with
// groups of 8 equal parts, d 768, k 100 (profiles/part_group): fused wins up
// to 131072 rows at nq 1 and nq 16, the per-part route (bf16 pre-filter, half
// the bytes) from 262144 rows at nq 1 and from 524288 at nq 16
static std::atomic<int64_t> g_group_rows{131072};
// the batch route (mqvs_set_part_group_batch): row limit in the low 32 bits
// (0 = off, the default), max_nq above them (0 = no cap) -- one word, so a
// search reads a pair some call set
static std::atomic<int64_t> g_group_batch{0};
// the fused route's row limit for binary parts (mqvs_set_part_group_binary_rows).
// Up to 32768 rows search_binary itself probes the whole part densely (P = n,
// search_binary.hip), so the fused route does the same device work per part
// with fewer launches and no host wait per part.  Above that it was measured
// with groups of 8 equal parts of 256-bit codes, k 100, Hamming and Jaccard
// (profiles/part_group/binary_limit.jsonl): fused wins at nq 1, 16 and 128 up
// to 131072 rows; at 262144 the per-part route (a short probe, then appends
// under its threshold) wins at nq 1, at 524288 at every nq
static std::atomic<int64_t> g_group_binary_rows{131072};
static thread_local mqvs_part_group_stats t_group_stats{};

static bool rows_fusable(const mqvs_segment *s, int64_t limit) { return !s->rows_host && s->n <= limit; }

static int64_t part_ords(const mqvs_segment *s) {
    return s->row_offset / s->granule + (s->n + s->granule - 1) / s->granule;
}

static mqvs_part_group *group_create(const mqvs_segment_t *segs, int nparts) {
    if (nparts < 1 || !segs) fail(MQVS_ERR_BAD_ARGUMENTS, "a part group needs at least one segment");
    for (int p = 0; p < nparts; ++p)
        if (!segs[p]) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment in a part group");
    for (int p = 0; p < nparts; ++p) {
        const mqvs_segment *s = segs[p];
        if (s->binary != segs[0]->binary)
            fail(MQVS_ERR_LOGICAL, "binary (FixedString) and Float32 segments in one part group");
        if (s->d != segs[0]->d) fail(MQVS_ERR_LOGICAL, "segments of a part group differ in dimension");
        // (a binary segment serves Hamming and Jaccard whatever its default metric)
        if (!s->binary && (s->metric == MQVS_METRIC_COSINE) != (segs[0]->metric == MQVS_METRIC_COSINE))
            fail(MQVS_ERR_LOGICAL, "cosine and non-cosine segments in one part group");
        if (s->device != segs[0]->device) fail(MQVS_ERR_BAD_ARGUMENTS, "segments of a part group are on different devices");
    }
    auto *g = new mqvs_part_group();
    g->segs.assign(segs, segs + nparts);
    g->device = segs[0]->device;
    g->d = segs[0]->d;
    g->binary = segs[0]->binary;
    g->cos = !g->binary && segs[0]->metric == MQVS_METRIC_COSINE;
    g->code_bytes = segs[0]->code_bytes;
    g->code_words = segs[0]->code_words;
    for (int p = 0; p < nparts; ++p) g->rows += segs[p]->n;
    return g;
}

// slots [first_slot, first_slot + nslots) (+ the sentinel) of one grouped
// scan + select: fused parts whose dense matrix fits the scratch budget
struct Slice {
    int first_slot, nslots;
    int64_t tiles, cols;
};
using PartGroupCall = GroupCall<GroupSlot, Slice>;

static std::vector<int64_t> part_rows(const mqvs_part_group *g) {
    std::vector<int64_t> rows;
    for (const mqvs_segment *seg : g->segs) rows.push_back(seg->n);
    return rows;
}

// the slices of a call's fused parts: a slice's dense [nq][cols] fp32 matrix
// fits the scratch budget.  fill(p, e) sets the part's own fields of its slot
// and returns its tiles
template <typename Fill>
static void build_part_slices(PartGroupCall &c, const mqvs_part_group *g, const std::vector<char> &fused, Fill &&fill) {
    const int64_t max_cols = std::max<int64_t>(1, (int64_t)(scratch_budget() / (sizeof(float) * (size_t)c.nq)));
    c.build_slices(
        fused, max_cols, [&](int p) { return g->segs[p]->n; },
        [&](int p, GroupSlot &e, Slice &cur) {
            const mqvs_segment *seg = g->segs[p];
            e.n = seg->n;
            e.granule = seg->granule;
            e.row_offset = seg->row_offset;
            e.tile0 = cur.tiles;
            e.col0 = cur.cols;
            cur.tiles += fill(p, e);
            cur.cols += seg->n;
        },
        [](GroupSlot &end, const Slice &cur) {
            end.tile0 = cur.tiles;
            end.col0 = cur.cols;
        });
}

// The fused slices of a call: the dense matrix sized to the widest slice; per
// slice the grouped scan (scan(p, slots, slice), skipped when the slice has
// no tiles), then the grouped select by `order`'s key into the per-part
// lists.  p: the scan's base parameters but for the matrix.
template <typename Scan>
static void scan_and_select(PartGroupCall &c, ScanParams &p, int order, int *fl, int32_t &launches, Scan &&scan) {
    int64_t ld = 0;
    for (const Slice &sl : c.slices) ld = std::max(ld, sl.cols);
    float *matrix = (float *)c.ws.pg_matrix.get(sizeof(float) * (size_t)c.nq * std::max<int64_t>(ld, 1));
    p.probe = matrix;
    for (const Slice &sl : c.slices) {
        const GroupSlot *slots = c.dslots + sl.first_slot;
        p.probe_ld = sl.cols;
        if (sl.tiles > 0) {
            scan(p, slots, sl);
            MQVS_HIP(hipGetLastError());
            launches += 1;
        }
        launch_select_group(matrix, sl.cols, slots, sl.nslots, c.nq, c.k, order, c.list_ids, c.list_dist, fl, c.s);
        MQVS_HIP(hipGetLastError());
        launches += 1;
    }
}

static void group_search(mqvs_part_group *g, const float *queries, int nq, int k, int metric,
                         const uint8_t *const *filters, const uint8_t *const *exists, int32_t *out_part,
                         int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t user_stream) {
    check_group_args(g, "part group",
                     g && g->binary ? "binary (FixedString) part group: search it with mqvs_part_group_search_binary"
                                    : nullptr,
                     nq, k, queries, out_part, out_ids, out_dist);
    const bool cos = metric == MQVS_METRIC_COSINE;
    if (metric != MQVS_METRIC_L2 && metric != MQVS_METRIC_IP && !cos)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Float32 Vector");
    if (cos != g->cos)
        fail(MQVS_ERR_LOGICAL, "part group was prepared for a different metric (cosine segments are "
                               "normalised in HBM and serve only cosine searches)");
    const int nparts = (int)g->segs.size();
    mqvs_part_group_stats st;
    if (!group_begin(nparts, nq, k, st, t_group_stats)) return;
    GroupScope sc(g->device, flags, user_stream);
    Workspace &ws = sc.ws;
    hipStream_t s = sc.s;
    const bool dev = flags & MQVS_F_DEVICE_PTRS;
    const int d = g->d;
    const int64_t qstride = round_up(d, 32);

    // ---- the routes.  Cosine: the variant table holds maxv variants per
    // query; a part of more chunk ordinals is fused only while the table
    // grown to them stays within the scratch budget (and kMaxVariantsCap)
    // batch: the call's nq selects faiss's BLAS formula -- its fused route is
    // the MFMA scan, and only when opted in
    const bool batch = nq >= kBlasThreshold;
    const int64_t batch_set = g_group_batch.load(std::memory_order_relaxed);
    const int64_t batch_rows = batch_set & 0xFFFFFFFF, batch_max_nq = batch_set >> 32;
    const bool route_on = !batch || (batch_rows > 0 && (batch_max_nq == 0 || nq <= batch_max_nq));
    const int64_t limit = batch ? batch_rows : g_group_rows.load(std::memory_order_relaxed);
    const int64_t tile_rows = batch ? kMfmaRows : kSmallRows;
    const int64_t maxv_fit =
        std::min<int64_t>(kMaxVariantsCap, (int64_t)(scratch_budget() / (sizeof(float) * (size_t)nq * qstride)));
    std::vector<char> fused(nparts, 0);
    int nfused = 0, maxv = cos ? kMaxVariants : 1;
    for (int p = 0; p < nparts; ++p) {
        const mqvs_segment *seg = g->segs[p];
        bool f = route_on && k <= kSortCap && rows_fusable(seg, limit);
        if (f && cos) {
            if (filters && filters[p]) f = false;  // (its chunk ordinals come from the filter)
            const int64_t o = part_ords(seg);
            if (o > kMaxVariants && o > maxv_fit) f = false;
            if (f) maxv = (int)std::max<int64_t>(maxv, o);
        }
        fused[p] = f;
        nfused += f;
        if (f) st.fused_rows += seg->n;
    }
    st.fused_parts = nfused;
    st.looped_parts = nparts - nfused;
    st.batch = batch && nfused > 0;

    // ---- inputs.  Host bitmaps: every part's into one pinned buffer behind
    // the slot tables, one copy to the device (GroupCall::stage)
    const float *dq =
        (const float *)ws.io.in(queries, sizeof(float) * (size_t)nq * d, nullptr, nullptr, 0, dev, s).queries;
    PartGroupCall c{part_rows(g), ws, s, dev, nq, k, filters, exists};
    build_part_slices(c, g, fused, [&](int p, GroupSlot &e) {
        const mqvs_segment *seg = g->segs[p];
        e.rows = seg->rows;
        e.row_norms = seg->norms;
        e.chunk_ord = seg->chunk_ord;
        e.nonempty = seg->nonempty_bits;
        // cosine and chunk-ordinal parts: tiles that never span two chunks
        const bool aligned = cos || seg->chunk_ord != nullptr;
        int64_t tiles = (seg->n + tile_rows - 1) / tile_rows;
        if (aligned && seg->n > 0) {
            // (a part shorter than its granule is one chunk: no tiles past its rows)
            e.tiles_per_chunk = (std::min(seg->granule, seg->n) + tile_rows - 1) / tile_rows;
            tiles = (seg->n + seg->granule - 1) / seg->granule * e.tiles_per_chunk;
        }
        return tiles;
    });
    c.stage(nullptr, 0);
    c.lists_and_outputs(out_part, out_ids, out_dist);

    // ---- the fused route
    if (nfused > 0) {
        // [overflow 4][status 4][qmu nq][qlam nq][qnorms nq]
        int *fl = (int *)ws.pg_q.get(sizeof(int) * (8 + 3 * (size_t)nq));
        launch_fill2((uint32_t *)fl, 8, 0u, nullptr, 0, 0u, s);
        int *qmu = fl + 8, *qlam = qmu + nq;
        float *qnorms = (float *)(qlam + nq);
        float *qvars = (float *)ws.pg_qvars.get(sizeof(float) * (size_t)nq * maxv * qstride);
        // (a chain that does not repeat within maxv steps sets fl[4]: every
        // fused part has at most maxv chunk ordinals, so none reads past it)
        launch_query_prep(dq, nq, d, cos ? MQVS_METRIC_COSINE : MQVS_METRIC_L2, batch && metric == MQVS_METRIC_L2, qvars,
                          maxv, qnorms, qmu, qlam, fl + 4, s);
        MQVS_HIP(hipGetLastError());
        st.launches += 2;
        ScanParams p{};
        p.d = d;
        p.nq = nq;
        p.qvars = qvars;
        p.qnorms = qnorms;
        p.qmu = qmu;
        p.qlam = qlam;
        p.maxv = maxv;
        p.blas_nq = nq;
        p.num_qblocks = (nq + kMfmaQ - 1) / kMfmaQ;
        scan_and_select(c, p, metric, fl, st.launches, [&](const ScanParams &sp, const GroupSlot *slots, const Slice &sl) {
            if (batch)
                launch_scan_group_mfma(sp, slots, sl.nslots, sl.tiles, metric, s);
            else
                launch_scan_group(sp, slots, sl.nslots, sl.tiles, metric, s);
        });
    }

    // ---- the per-part route (each search ends in its own host wait)
    for (int p = 0; p < nparts; ++p) {
        if (fused[p]) continue;
        search_segment(g->segs[p], dq, nq, k, metric, c.part_filter(p), c.part_exists(p), c.part_ids(p),
                       c.part_dist(p), flags & ~(uint32_t)MQVS_F_ASYNC, s, -1);
    }

    // ---- the merge, and the call's one wait
    c.merge_and_wait(metric, out_part, st.launches);
    st.total_ms = sc.total_ms();
    t_group_stats = st;
}

// mqvs_part_group_search_binary: the same call over binary parts.  Both binary
// distances are ascending and finite, so select and merge run with the L2
// order (as search_binary's own selects and mqvs_merge_shards do); there is no
// formula switch at nq 20 and no chunk arithmetic, so one fused route serves
// every nq and a filter never sends a part to the per-part route.
static void group_search_binary(mqvs_part_group *g, const uint8_t *queries, int nq, int k, int metric,
                                const uint8_t *const *filters, const uint8_t *const *exists, int32_t *out_part,
                                int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t user_stream) {
    check_group_args(g, "part group",
                     g && !g->binary ? "Float32 part group: search it with mqvs_part_group_search" : nullptr, nq, k,
                     queries, out_part, out_ids, out_dist);
    if (metric != MQVS_METRIC_HAMMING && metric != MQVS_METRIC_JACCARD)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Binary Vector");
    const int nparts = (int)g->segs.size();
    mqvs_part_group_stats st;
    if (!group_begin(nparts, nq, k, st, t_group_stats)) return;
    GroupScope sc(g->device, flags, user_stream);
    Workspace &ws = sc.ws;
    hipStream_t s = sc.s;
    const bool dev = flags & MQVS_F_DEVICE_PTRS;
    constexpr int kOrder = MQVS_METRIC_L2;  // ascending finite values: ord_asc key, (key, row) ties

    // ---- the routes
    const int64_t limit = g_group_binary_rows.load(std::memory_order_relaxed);
    std::vector<char> fused(nparts, 0);
    int nfused = 0;
    for (int p = 0; p < nparts; ++p) {
        fused[p] = k <= kSortCap && rows_fusable(g->segs[p], limit);
        nfused += fused[p];
        if (fused[p]) st.fused_rows += g->segs[p]->n;
    }
    st.fused_parts = nfused;
    st.looped_parts = nparts - nfused;

    // ---- inputs.  The host queries ride with the slot tables and bitmaps
    PartGroupCall c{part_rows(g), ws, s, dev, nq, k, filters, exists};
    build_part_slices(c, g, fused, [&](int p, GroupSlot &e) {
        e.codes = g->segs[p]->codes;
        return (e.n + kSmallRows - 1) / kSmallRows;  // plain tiles from row 0 (no chunk arithmetic)
    });
    c.stage(dev ? nullptr : queries, dev ? 0 : (size_t)nq * g->code_bytes);
    const uint8_t *dq = dev ? queries : c.dextra;  // [nq][code_bytes] on the device
    c.lists_and_outputs(out_part, out_ids, out_dist);

    // ---- the fused route
    if (nfused > 0) {
        int *fl = (int *)ws.pg_q.get(sizeof(int) * 8);  // [overflow 4][unused 4]
        launch_fill2((uint32_t *)fl, 8, 0u, nullptr, 0, 0u, s);
        MQVS_HIP(hipGetLastError());
        st.launches += 1;
        // the query codes, zero padded to the segments' row stride, once per call
        uint32_t *qc = (uint32_t *)ws.pg_qvars.get((size_t)nq * g->code_words * 4);
        upload_codes(qc, g->code_words, dq, g->code_bytes, nq, true, s);
        ScanParams p{};
        p.d = g->d;
        p.nq = nq;
        p.qcodes = qc;
        p.code_words = g->code_words;
        p.nbits = g->d;
        scan_and_select(c, p, kOrder, fl, st.launches, [&](const ScanParams &sp, const GroupSlot *slots, const Slice &sl) {
            launch_scan_group_binary(sp, slots, sl.nslots, sl.tiles, metric, s);
        });
    }

    // ---- the per-part route (each search ends in its own host wait)
    for (int p = 0; p < nparts; ++p) {
        if (fused[p]) continue;
        search_binary(g->segs[p], dq, nq, k, metric, c.part_filter(p), c.part_exists(p), c.part_ids(p), c.part_dist(p),
                      (flags & ~(uint32_t)MQVS_F_ASYNC) | (uint32_t)MQVS_F_DEVICE_PTRS, s);
    }

    // ---- the merge, and the call's one wait
    c.merge_and_wait(kOrder, out_part, st.launches);
    st.total_ms = sc.total_ms();
    t_group_stats = st;
}

}  // namespace mqvs

using namespace mqvs;

extern "C" {

int mqvs_part_group_create(const mqvs_segment_t *segs, int32_t nparts, mqvs_part_group_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        *out = group_create(segs, nparts);
    });
}

int mqvs_part_group_free(mqvs_part_group_t group) {
    return guarded([&] { delete group; });
}

int mqvs_part_group_info(mqvs_part_group_t group, int32_t *nparts, int64_t *rows, int32_t *d, int32_t *fusable_parts,
                         size_t *hbm_bytes) {
    return guarded([&] {
        if (!group) fail(MQVS_ERR_BAD_ARGUMENTS, "null part group");
        if (nparts) *nparts = (int32_t)group->segs.size();
        if (rows) *rows = group->rows;
        if (d) *d = group->d;
        if (fusable_parts) {
            const int64_t limit = (group->binary ? g_group_binary_rows : g_group_rows).load(std::memory_order_relaxed);
            int32_t f = 0;
            for (const mqvs_segment *s : group->segs) f += rows_fusable(s, limit);
            *fusable_parts = f;
        }
        if (hbm_bytes) *hbm_bytes = 0;
    });
}

int mqvs_part_group_search(mqvs_part_group_t group, const float *queries, int32_t nq, int32_t k, int32_t metric,
                           const uint8_t *const *filters, const uint8_t *const *row_exists, int32_t *out_part,
                           int64_t *out_ids, float *out_dist, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{9, (uint64_t)(uintptr_t)group, (uint64_t)nq, (uint64_t)k, (uint64_t)metric, filters != nullptr,
                      row_exists != nullptr, flags};
        group_search(group, queries, nq, k, metric, filters, row_exists, out_part, out_ids, out_dist, flags,
                     (hipStream_t)stream);
    });
}

int mqvs_part_group_search_binary(mqvs_part_group_t group, const uint8_t *queries, int32_t nq, int32_t k,
                                  int32_t metric, const uint8_t *const *filters, const uint8_t *const *row_exists,
                                  int32_t *out_part, int64_t *out_ids, float *out_dist, uint32_t flags,
                                  mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{10, (uint64_t)(uintptr_t)group, (uint64_t)nq, (uint64_t)k, (uint64_t)metric, filters != nullptr,
                      row_exists != nullptr, flags};
        group_search_binary(group, queries, nq, k, metric, filters, row_exists, out_part, out_ids, out_dist, flags,
                            (hipStream_t)stream);
    });
}

int mqvs_part_group_last_stats(mqvs_part_group_stats *out) {
    if (!out) return MQVS_ERR_BAD_ARGUMENTS;
    *out = t_group_stats;
    return MQVS_OK;
}

int mqvs_set_part_group_batch(int64_t rows, int32_t max_nq) {
    if (rows < 0 || rows > kGroupRowsMax || max_nq < 0 || (max_nq > 0 && max_nq < kBlasThreshold))
        return MQVS_ERR_BAD_ARGUMENTS;
    g_group_batch.store(rows | ((int64_t)max_nq << 32), std::memory_order_relaxed);
    return MQVS_OK;
}

int mqvs_part_group_batch(int64_t *rows, int32_t *max_nq) {
    const int64_t v = g_group_batch.load(std::memory_order_relaxed);
    if (rows) *rows = v & 0xFFFFFFFF;
    if (max_nq) *max_nq = (int32_t)(v >> 32);
    return MQVS_OK;
}

int64_t mqvs_set_part_group_rows(int64_t rows) {
    const int64_t prev = g_group_rows.load(std::memory_order_relaxed);
    if (rows > 0) g_group_rows.store(std::min<int64_t>(rows, kGroupRowsMax), std::memory_order_relaxed);
    return prev;
}

int64_t mqvs_set_part_group_binary_rows(int64_t rows) {
    const int64_t prev = g_group_binary_rows.load(std::memory_order_relaxed);
    if (rows > 0) g_group_binary_rows.store(std::min<int64_t>(rows, kGroupRowsMax), std::memory_order_relaxed);
    return prev;
}

}  // extern "C"
