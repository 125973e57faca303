// search.hip -- the FLAT search of a float segment, and the exact re-rank.
//
// Search = the whole of MergeTreeVSManager::vectorScanWithoutIndex for one data
// part (MergeTreeVSManager.cpp:960-1536) in a handful of launches:
//   1. query prep        (norms; cosine re-normalisation variants)
//   2. probe scan        dense values for rows [0, P) (P ~ 3k*n/4096)
//   3. probe select      per-query k-th key -> threshold tau; first candidates
//   4. main scan         rows [P, n), append rows with key <= tau
//   5. final select      sort candidates by the reference's total order, emit k
// If a candidate list overflows (mass ties; rows ordered by distance to the
// queries), the stored candidates and tau are discarded and the part is
// re-scanned from an empty list in short segments with a refinement after
// each (rescan_on_overflow; counted in the stats).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <string>

#include "workspace.h"

namespace mqvs {

struct Range {
    int64_t begin, end, tiles, tiles_per_chunk;
};

static Range make_range(int64_t b, int64_t e, int64_t tile_rows, int64_t chunk_rows, bool aligned) {
    Range r{b, e, 0, 0};
    if (e <= b) return r;
    if (aligned) {
        r.tiles_per_chunk = (chunk_rows + tile_rows - 1) / tile_rows;
        const int64_t nch = (e - b + chunk_rows - 1) / chunk_rows;
        r.tiles = nch * r.tiles_per_chunk;
    } else {
        r.tiles = (e - b + tile_rows - 1) / tile_rows;
    }
    return r;
}

enum ScanKind { kScanSmall = 0, kScanMfma32 = 1, kScanBf16 = 2 };

// tile_rows: the range's tile length when not the kind's (kBfRowsSmall: a
// bf16 scan that scan_hi_small_tiles_ok admits)
static void run_scan(ScanParams p, const Range &r, int kind, int metric, bool probe, hipStream_t st,
                     int64_t tile_rows = 0) {
    if (r.tiles <= 0) return;
    p.row_begin = r.begin;
    p.row_end = r.end;
    p.tiles = r.tiles;
    p.tiles_per_chunk = r.tiles_per_chunk;
    p.tile_rows = tile_rows > 0 ? tile_rows : kind == kScanSmall ? kSmallRows : kind == kScanBf16 ? kBfRows : kMfmaRows;
    if (kind == kScanMfma32)
        launch_scan_mfma(p, metric, probe, st);
    else if (kind == kScanBf16)
        launch_scan_hi(p, metric, probe, st);
    else
        launch_scan_small(p, metric, probe, st);
    MQVS_HIP(hipGetLastError());
}

// Query variants.  Cosine re-normalises the query once per searched chunk
// (VIWithDataPart.h:358, the query object shared across chunks); the chain
// x, x/|x|, ... is stored until it repeats (mu, lambda per query).  The
// default table of kMaxVariants covers the chains of typical data (Gaussian
// and mixture parts repeat within ~15 steps).  When a part has more chunk
// ordinals than that and some chain did not repeat (small-integer vectors
// wander for hundreds of steps), the table is rebuilt with one variant per
// ordinal (up to kMaxVariantsCap) -- one host sync, only on such parts.
// Returns maxv; ASYNC calls cannot sync and keep the default table (their
// outcome goes to mqvs_async_check).
// zeroed_status: 4 ints the caller has already zeroed on this stream (saves a
// memset launch), or null
static int prep_variants(Workspace &ws, const float *dq, int nq, int d, bool cos, bool l2norms, int64_t ords,
                         bool may_sync, float *&qvars, float *&qnorms, int *&qmu, int *&qlam, int *&status,
                         hipStream_t s, int *zeroed_status = nullptr, int maxv_override = 0) {
    const int64_t qstride = round_up(d, 32);
    qnorms = (float *)ws.qnorms.get(sizeof(float) * nq);
    qmu = (int *)ws.qmu.get(sizeof(int) * nq);
    qlam = (int *)ws.qlam.get(sizeof(int) * nq);
    status = zeroed_status ? zeroed_status : (int *)ws.status.get(sizeof(int) * 4);
    int maxv = cos ? (maxv_override > 0 ? maxv_override : kMaxVariants) : 1;
    for (int pass = 0; pass < 2; ++pass) {
        const size_t bytes = sizeof(float) * (size_t)nq * maxv * qstride;
        // (no clear of the table: the prep writes every stored variant,
        // zeros past a query's chain)
        qvars = (float *)ws.qvars.get(bytes);
        if (pass > 0 || !zeroed_status) launch_fill2((uint32_t *)status, 4, 0u, nullptr, 0, 0u, s);
        launch_query_prep(dq, nq, d, cos ? MQVS_METRIC_COSINE : MQVS_METRIC_L2, l2norms, qvars, maxv, qnorms, qmu,
                          qlam, status, s);
        MQVS_HIP(hipGetLastError());
        if (pass > 0 || !cos || ords <= maxv || !may_sync || maxv_override > 0) break;
        MQVS_HIP(hipMemcpyAsync(ws.host_flags + 12, status, sizeof(int), hipMemcpyDeviceToHost, s));
        host_wait(s);
        if (!ws.host_flags[12]) break;
        maxv = (int)std::min<int64_t>(ords, kMaxVariantsCap);
    }
    return maxv;
}

// the gather list launched before the selected count is read
// (FlatSearch::choose_gather) is sized for every row: up to 64M rows' worth
constexpr size_t kSpecListBytes = (size_t)256 << 20;

// Main-scan segmentation: the first segment is `first` probe lengths, each
// next one `growth` times the previous; the probe aims at `target`
// candidates.  Few queries: fewer, longer segments (each refinement is a
// launch boundary plus a one-workgroup kernel; measured at 10M x 768, nq 1:
// 7 segments 2.81 ms, 3 segments 2.72 ms; nq 1000 prefers 2, 2).
// MQVS_SEG="first,growth,target" overrides (tools/ab_split.py).
constexpr int64_t kMinSegRows = 65536;
struct SegTune {
    int64_t first = 2, growth = 2, target = 16384;
};
static SegTune seg_tune(int nq) {
    SegTune v;
    if (nq <= 4) {
        v.first = 8;
        v.growth = 4;
        // one or two queries: a 4x shorter probe (its single-workgroup select
        // 53 -> 21 us at 10M x 768; one more segment; wall median 2.80 ->
        // 2.75 ms at nq 1, no gain at nq 4, profiles/r02/smallnq/seg_ab.jsonl);
        // round 6: half that probe and a first segment of 16 probe lengths
        // (3 segments, 2 refinements): kernels 2.386 -> 2.365 ms, wall median
        // 2.418-2.439 -> 2.394-2.404 ms (profiles/r06/seg_ab_nq1.jsonl)
        if (nq <= 2) {
            v.first = 16;
            v.target = 32768;
        }
    } else if (nq < 256) {
        v.first = 4;
        v.growth = 4;
    }
    if (const char *e = tune_env("MQVS_SEG")) {
        long long a = 0, b = 0, c = 0;
        if (std::sscanf(e, "%lld,%lld,%lld", &a, &b, &c) == 3 && a >= 1 && b >= 2 && c >= 256) {
            v.first = a;
            v.growth = b;
            v.target = c;
        }
    }
    return v;
}

// One mqvs_search call.  metric: public metric, or kMetricIpRaw for the
// faiss-contract entry point.
// formula_nq: the batch size that selects faiss's distance formula (0: nq).
// Query sub-batches of one call (large k) keep the call's formula: faiss
// decides it from the whole batch (BruteForceSearch.h:80-87, nx >= 20).
// async_word (ASYNC calls only): where the search's fallback flags go instead
// of the thread's sticky word (the sharded search exchanges them); the
// survivor counts and event times are then collected by search_collect_stats
// after the caller's own stream sync.
struct FlatArgs {
    mqvs_segment *seg;
    const float *queries;
    int nq, k, metric;
    const uint8_t *filter, *exists;
    int64_t *out_ids;
    float *out_dist;
    uint32_t flags;
    hipStream_t user_stream;
    bool force_exact = false;
    int64_t ord_base = -1;
    int maxv_hint = 0;
    int formula_nq = 0;
    int *async_word = nullptr;
};

static void search_impl(const FlatArgs &a);

// The search of one query batch as stages over its state: run() queues them in
// order on one stream.  Every stage reads what earlier ones left in the
// members; nothing here outlives the call (the buffers are the workspace's).
struct FlatSearch {
    // ---- call inputs
    const FlatArgs &a;
    Workspace &ws;
    const hipStream_t s;
    mqvs_segment *const seg;
    const int nq, k, metric;
    const int fnq;  // the batch size that selects faiss's formula
    // ---- derived constants
    const int64_t n;
    const int d;
    const int64_t bm_bytes;
    const bool dev, async, timing, cos;
    const int batch_mode, gather_mode;
    // a filtered search waits for its selected-row count mid-call: behind
    // earlier work on the caller's stream (e.g. ASYNC searches) it sleeps
    // instead of spinning (choose_gather)
    const bool queued_on_entry;
    const bool mfma, bf16_ok;
    // Cosine pads each chunk's run to whole tiles (a tile's query variant is
    // its chunk's); L2 / IP have one variant, so their list is dense and only
    // its end is padded (at 1 % selectivity per-chunk padding made the list
    // 3x the selected rows: 82 rows per 8192-row chunk, padded to 256)
    const int gtile;
    const int64_t nch;   // granule chunks of the part
    const int64_t ords;  // chunk ordinals the part's searches reach
    bool bf16 = false;
    int kind = kScanSmall, cap = 0, maxv = 1;
    // ---- device pointers
    const float *dq = nullptr;
    const uint8_t *dfilter = nullptr, *dexists = nullptr;
    CallIO::Out out{};
    int *fl = nullptr;  // one zeroed block: [overflow 4][status 4][count nq][gather-count ticket 1]
    int *overflow = nullptr, *status = nullptr, *count = nullptr;
    int *gcount = nullptr;
    int64_t *goff = nullptr;
    float *qvars = nullptr;
    int *qmu = nullptr, *qlam = nullptr;
    uint32_t *tau = nullptr;
    Cand *cand = nullptr, *cand_alt = nullptr;  // the lists; what the refinements compact them into
    int *count_alt = nullptr;
    float *bq = nullptr, *probe = nullptr;
    uint4 *large = nullptr;
    int32_t *spec_list = nullptr;
    ScanParams p{};
    // ---- the plan
    int64_t selected = -1, gpadded = 0;  // rows that pass the filter (-1: not counted), their padded list
    const int32_t *row_list = nullptr;
    int64_t scan_n = 0;  // scan positions: rows, or gather-list entries
    bool aligned = false;
    int64_t tile_rows = 0, ptile = 0, P = 0;
    SegTune tune;
    Range pr{};
    bool bprobe = false;
    int64_t probe_cols = 0, probe_ld = 0;
    bool flags_folded = false;  // the status words stored by the final select (k_sort_emit)
    int seg_events = 0;         // main-scan segments with timing events
    // (armed between the count launch and the host's read of its totals: an
    // exception in between drains the stream, so that no count kernel of this
    // call is still in flight when the next call on this workspace rearms the
    // pinned record)
    struct CountDrain {
        hipStream_t s = nullptr;
        ~CountDrain() {
            if (s) (void)hipStreamSynchronize(s);
        }
    } count_drain;
    int64_t count_gen = 0;
    // ---- stats
    mqvs_search_stats st{};

    FlatSearch(const FlatArgs &args, Workspace &w, hipStream_t stream)
        : a(args), ws(w), s(stream), seg(args.seg), nq(args.nq), k(args.k), metric(args.metric),
          fnq(args.formula_nq > 0 ? args.formula_nq : args.nq), n(seg->n), d(seg->d), bm_bytes((n + 7) / 8),
          dev(args.flags & MQVS_F_DEVICE_PTRS), async(dev && (args.flags & MQVS_F_ASYNC)),
          timing(timing_on(args.flags)), cos(metric == MQVS_METRIC_COSINE), batch_mode(call_batch_mode(args.flags)),
          gather_mode(call_gather_mode(args.flags)),
          queued_on_entry(args.filter && hipStreamQuery(s) == hipErrorNotReady), mfma(fnq >= kBlasThreshold),
          bf16_ok(seg->approx_ok && !args.force_exact && batch_mode == 0), gtile(cos ? (int)kSmallRows : 1),
          nch((n + seg->granule - 1) / seg->granule),
          ords((args.ord_base >= 0 ? args.ord_base : seg->row_offset / seg->granule) + nch) {}

    void stage_inputs();
    void start_count();
    void prep_queries();
    void choose_gather();
    void plan_probe();
    void run_probe();
    void run_segments();
    void final_select();
    void finish_async();
    void finish_sync();

    void run() {
        stage_inputs();
        start_count();
        prep_queries();
        choose_gather();
        plan_probe();
        run_probe();
        run_segments();
        final_select();
        if (async)
            finish_async();
        else
            finish_sync();
    }
};

void FlatSearch::stage_inputs() {
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[0], s));
    const CallIO::In in = ws.io.in(a.queries, sizeof(float) * (size_t)nq * d, a.filter, a.exists, bm_bytes, dev, s);
    dq = (const float *)in.queries;
    dfilter = in.filter;
    dexists = in.exists;
    out = ws.io.out((size_t)nq * k, dev, a.out_ids, a.out_dist);
}

// ---- selective PREWHERE: count the rows that pass (filter, non-empty,
// not deleted); a selective scan then walks a gather list of just those
// rows (per chunk in row order, padded to whole tiles) and reads
// selectivity x n rows instead of all of them
void FlatSearch::start_count() {
    static_assert(kSmallRows == kBfRows, "gather-list padding is one tile of either kernel");
    // one zeroed block for the status words: [overflow 4][status 4][count nq]
    // [gather-count ticket 1]
    fl = (int *)ws.flags.get(sizeof(int) * (9 + (size_t)nq));
    launch_fill2((uint32_t *)fl, 9 + (int64_t)nq, 0u, nullptr, 0, 0u, s);
    overflow = fl;
    count = fl + 8;  // zeroed with the status words
    if (!(dfilter && gather_mode != 0 && n > 0)) return;
    gcount = (int *)ws.gcount.get(sizeof(int) * nch);
    goff = (int64_t *)ws.goff.get(sizeof(int64_t) * (nch + 2));
    // the totals also land in pinned host memory (k_chunk_count), read once
    // the query prep, chunk ordinals and bf16 query planes are queued: the
    // host waits for this kernel only, not for a drained stream.  The
    // record [padded, selected, generation] is this call's once its
    // generation word (written last, behind a system-scope fence) shows
    // this call's number.
    auto *htot = reinterpret_cast<int64_t *>(ws.host_flags + kCountRec);
    count_gen = ++ws.count_gen;
    htot[2] = 0;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    launch_gather_count(dfilter, seg->nonempty_bits, dexists, n, seg->granule, gtile, gcount, goff, goff + nch, htot,
                        count_gen, fl + 8 + nq, s);
    MQVS_HIP(hipGetLastError());
    count_drain.s = s;
    selected = 0;
    fault_point_mid();
}

void FlatSearch::prep_queries() {
    // ---- query prep
    const int64_t qstride = round_up(d, 32);
    float *qnorms = nullptr;
    // The query-variant table starts at kMaxVariants per query without a host
    // round trip; a chain that does not repeat within it on a part of more
    // chunk ordinals (rare: small-integer data) is caught from the status word
    // read at the end, and the search re-runs with the larger table.  (The
    // kernel choice below never changes bf16 from bf16_ok.)
    maxv = prep_variants(ws, dq, nq, d, cos, (mfma || bf16_ok) && metric == MQVS_METRIC_L2, ords, false, qvars, qnorms,
                         qmu, qlam, status, s, fl + 4, a.maxv_hint);

    // ---- chunk ordinals
    const int *chunk_ord = nullptr;
    if (dfilter) {
        if (cos) {
            int *o = (int *)ws.ord.get(sizeof(int) * std::max<int64_t>(nch, 1));
            launch_chunk_ordinals(dfilter, seg->nonempty_bits, dexists, n, seg->granule, 1, o, s);
            MQVS_HIP(hipGetLastError());
            chunk_ord = o;
        }
    } else {
        chunk_ord = seg->chunk_ord;
    }
    // ---- kernel choice
    // faiss's formula branch is set by nq (kBlasThreshold); the bf16
    // pre-filter serves both branches (its exact re-rank uses the branch's
    // formula) whenever the segment has its plane, the exact kernels the rest.  A
    // gathered (selective) scan prefers the bf16 kernel at any nq: its LDS-DMA
    // keeps whole tiles of scattered rows in flight and gathers efficiently up
    // to ~60% selectivity, while the VALU kernel's 128-B row slices only pay
    // below ~30% (tools/sweep.py --sels, profiles/r01)
    // (the bf16 plane streams half the bytes of the fp32 rows, so it serves
    // every batch size)
    // (the gather decision below never changes bf16 from bf16_ok, so the kind
    // and the bf16 query planes are set before the selected count is known)
    bf16 = bf16_ok;
    kind = bf16 ? kScanBf16 : !mfma ? kScanSmall : kScanMfma32;

    // ---- candidate capacity per query (a fixed budget spread over the batch)
    cap = cand_capacity(nq, k);

    p.rows = seg->rows;
    p.row_norms = seg->norms;
    p.n = n;
    p.d = d;
    p.nq = nq;
    p.qvars = qvars;
    p.qnorms = qnorms;
    p.qmu = qmu;
    p.qlam = qlam;
    p.maxv = maxv;
    p.chunk_rows = seg->granule;
    p.chunk_ord = chunk_ord;
    // a row-range shard of a part continues the part's chunk ordinals (all
    // earlier chunks assumed searched; see DESIGN.md, cosine + shards)
    p.ord_base = (int)(a.ord_base >= 0 ? a.ord_base : seg->row_offset / seg->granule);
    p.filter = dfilter;
    p.exists = dexists;
    p.nonempty = seg->nonempty_bits;
    p.num_qblocks = (nq + kMfmaQ - 1) / kMfmaQ;
    p.blas_nq = fnq;
    tau = (uint32_t *)ws.tau.get(sizeof(uint32_t) * nq);
    cand = (Cand *)ws.cand.get(sizeof(Cand) * (size_t)nq * cap);
    p.tau = tau;
    p.cand_count = count;
    p.cand = cand;
    p.cand_cap = cap;

    if (kind != kScanBf16) return;
    // bf16 plane of the query variants + per-query error bound
    const int64_t nvec = (int64_t)nq * maxv;
    bq = (float *)ws.bq.get(sizeof(float) * nq);
    p.rows_hi = seg->rows_hi;
    p.dpad = seg->dpad;
    p.thr = (const float *)ws.thr.get(sizeof(float) * nq);
    p.split = seg->split;
    // batch scans (kernels_p4.hip): per-wave candidate queues
    if (nq > 128) p.p4_queue = ws.p4q.get(p4_queue_bytes());
    // [hi: maxv x vpad x dpad x 2 B][records: nvec x kMxRec floats]
    const int64_t vpad = round_up(nq, 16);
    const int64_t pvec = (int64_t)maxv * vpad;
    const size_t o_rec = (size_t)round_up(pvec * seg->dpad * 2, 256);
    auto *base = (unsigned char *)ws.qhi.get(o_rec + sizeof(float) * kMxRec * (size_t)nvec);
    auto *qhi = (uint16_t *)base;
    auto *qrec = (float *)(base + o_rec);
    launch_to_hi(qvars, nvec, d, qstride, seg->dpad, maxv, vpad, qhi, qrec, nullptr, s);
    p.q_vpad = vpad;
    p.q_hi = qhi;
    launch_query_bound(p, metric, seg->ynorm_max, qrec, seg->ynorm_max + 4, bq, overflow, s);
    // cosine batches: a chunk's query variants as one contiguous plane
    // (kernels_p4.hip; up to 32 planes within the scratch budget; the
    // scan keeps per-query variant reads when the chains need more)
    const int64_t plane = vpad * seg->dpad * 2;
    const int pcap = (int)std::min<int64_t>({kP4OrdPlanesMax, maxv, (int64_t)(scratch_budget() / plane)});
    if (p.p4_queue && metric == MQVS_METRIC_COSINE && maxv > 1 && pcap >= 2 && tune_int("MQVS_P4_ORD", 1)) {
        const size_t pb = (size_t)round_up((int64_t)pcap * plane, 256);
        auto *ob = (unsigned char *)ws.qord.get(pb + 256);
        auto *desc = (int *)(ob + pb);
        launch_ord_planes(qhi, (uint16_t *)ob, desc, qmu, qlam, nq, vpad, seg->dpad, pcap, s);
        p.q_ord = (const uint16_t *)ob;
        p.q_ord_desc = desc;
    }
    MQVS_HIP(hipGetLastError());
}

void FlatSearch::choose_gather() {
    // ---- the gather list, launched before the host reads the count (when
    // the call may gather): k_compact_rows needs only the device offsets, and
    // pads the list's end from the device totals, so the host's round trip
    // for the count overlaps it.  Sized for every row (n entries plus the
    // chunks' tile padding); a search the count then sends to the mask scan
    // wasted one compaction beside a scan of >= 60 % of the part.
    // (Parts whose worst-case list passes kSpecListBytes -- 64M rows -- keep
    // the list sized by the count: the workspace peak is what admission
    // reserves for the thread's next call.)
    const int64_t worst = round_up(n + nch * (int64_t)(gtile - 1), kSmallRows);
    if (selected >= 0 && (gather_mode == 2 || bf16_ok || (!bf16 && !mfma)) &&
        (size_t)worst * sizeof(int32_t) <= kSpecListBytes) {
        spec_list = (int32_t *)ws.glist.get(sizeof(int32_t) * (size_t)std::max<int64_t>(worst, 1));
        launch_gather_list(dfilter, seg->nonempty_bits, dexists, n, seg->granule, gtile, gcount, goff, spec_list, -1, s,
                           goff + nch, kSmallRows);
        MQVS_HIP(hipGetLastError());
    }

    // ---- the selected count (k_chunk_count's pinned record, polled with a
    // pause for up to kCountSpinUs; then -- or at once behind earlier work on
    // the caller's stream, or in MQVS_WAIT_BLOCK -- the host's wait)
    if (selected >= 0) {
        volatile int64_t *htot = reinterpret_cast<volatile int64_t *>(ws.host_flags + kCountRec);
        const int spin = queued_on_entry || wait_spin_us() == 0 ? 0 : kCountSpinUs;
        const auto t0 = std::chrono::steady_clock::now();
        while (htot[2] != count_gen) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin)) {
                host_wait(s);
                break;
            }
            for (int i = 0; i < 8; ++i) cpu_relax();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        int64_t tot[2] = {htot[0], htot[1]};
        if (htot[2] != count_gen) {
            // (the pinned record never showed: the device totals, the stream drained)
            MQVS_HIP(hipMemcpyAsync(tot, goff + nch, sizeof(tot), hipMemcpyDeviceToHost, s));
            host_wait(s);
        }
        count_drain.s = nullptr;
        gpadded = round_up(tot[0], kSmallRows);
        selected = tot[1];
    }
    bool gather = false;
    if (selected >= 0) {
        if (gather_mode == 2)
            gather = bf16 || !mfma;
        else if (bf16_ok && 10 * selected <= 6 * n)
            gather = true;
        else if (!bf16 && !mfma && 10 * selected <= 3 * n)
            gather = true;
    }

    // ---- gather list of the selected rows
    scan_n = n;
    if (gather) {
        int32_t *list = spec_list;
        if (!list) {
            list = (int32_t *)ws.glist.get(sizeof(int32_t) * std::max<int64_t>(gpadded, 1));
            // (the list's tail up to gpadded: -1 entries, written by the last chunk)
            launch_gather_list(dfilter, seg->nonempty_bits, dexists, n, seg->granule, gtile, gcount, goff, list,
                               gpadded, s);
            MQVS_HIP(hipGetLastError());
        }
        row_list = list;
        scan_n = gpadded;
        st.gather = 1;
    }
    aligned = !row_list && (cos || p.chunk_ord != nullptr);
    tile_rows = kind == kScanBf16 ? kBfRows : !mfma ? kSmallRows : kMfmaRows;
    p.row_list = row_list;
}

void FlatSearch::plan_probe() {
    // ---- probe size: expected candidates ~ k*n/P; aim at cap/3
    // (more candidates = more appends from the scan; 16k keeps them cheap)
    tune = seg_tune(nq);
    const int64_t target_cands = std::min<int64_t>(cap / 3, std::max<int64_t>(tune.target, 2 * (int64_t)k));
    large = k > kSortCap ? (uint4 *)ws.large.get(sizeof(uint4) * 2 * kLargeCap * (size_t)nq) : nullptr;
    P = scan_n;
    // (small k over a part much larger than k -- e.g. the index build's
    // top-1 k-means assignment against 10^4 centroids -- also takes a short
    // probe: a dense probe of every row would dominate the search)
    if (scan_n > 32768 || (k <= 16 && scan_n > 16 * tile_rows)) {
        P = (int64_t)(((double)k * (double)scan_n) / target_cands) + 1;
        // (a shorter probe is cheaper but its looser threshold sends more
        // waves of the first segments down the append path: measured net
        // loss at nq = 1000 with a 64 MB cap on the probe matrix)
        P = std::max<int64_t>(P, 8 * (int64_t)k);
        // A gathered scan's appends take the per-row path (list lookup,
        // bitmap tests, norms), so a loose first threshold is costly there:
        // at 1 % of 50M rows a 1024-position probe left ~10 % of the first
        // segment's rows passing (110 us for 66k positions, then a 45 us
        // refinement).  A probe of scan_n / 16 positions (<= 16384) costs
        // about the same launch and cuts the first segment's appends ~16x.
        if (row_list) P = std::max<int64_t>(P, std::min<int64_t>(scan_n / 16, 16384));
        P = round_up(P, aligned ? seg->granule : tile_rows);
        if (P > scan_n) P = scan_n;
    }

    // the dense probe of a few queries in kBfRowsSmall-row tiles: 4x the
    // workgroups (a 16384-position probe is 64 tiles of 256 -- a quarter of
    // the CUs, each wave walking four blocks in a row).  Gathered probes at
    // nq <= 16: 34 -> 17 us (1 % of 50M rows, nq 1: 0.447 -> 0.431 ms wall);
    // contiguous ones only at nq <= 2 (cosine 10M, nq 1: 15 -> 12 us; nq 16:
    // 23 -> 27 us), profiles/r05/small_tiles/
    ptile = (kind == kScanBf16 && (row_list || nq <= 2) && scan_hi_small_tiles_ok(nq, seg->dpad)) ? kBfRowsSmall
                                                                                                  : tile_rows;
    pr = make_range(0, P, ptile, seg->granule, aligned);
}

void FlatSearch::run_probe() {
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[5], s));
    (void)take_batch_kernel_flag();
    // The batch probe (kernels_p4.hip PROBE): the batch kernel over the probe
    // rows writes one best value per (query, 128-row half tile) instead of the
    // dense [nq][P] matrix; the threshold comes from the k-th of those maxima
    // and the main scan then starts at row 0 (the probe rows are re-scanned,
    // ~P / n of the main scan).  Otherwise the dense probe and its select,
    // which also appends the probe rows that pass.
    probe_cols = P;
    probe_ld = P;
    if (kind == kScanBf16 && p.p4_queue && !row_list && P < scan_n && pr.tiles > 0) {
        const int64_t gld = round_up(2 * pr.tiles, 4);
        probe = (float *)ws.probe.get(sizeof(float) * (size_t)nq * gld);
        ScanParams pp = p;
        pp.row_begin = pr.begin;
        pp.row_end = pr.end;
        pp.tiles = pr.tiles;
        pp.tiles_per_chunk = pr.tiles_per_chunk;
        pp.tile_rows = kBfRows;
        pp.p4_gmax = probe;
        pp.p4_gld = gld;
        bprobe = launch_scan_p4_probe(pp, metric, s);
        MQVS_HIP(hipGetLastError());
        if (bprobe) {
            probe_cols = 2 * pr.tiles;
            probe_ld = gld;
        }
    }
    if (!bprobe) {
        probe = (float *)ws.probe.get(sizeof(float) * (size_t)nq * P);
        p.probe = probe;
        p.probe_ld = P;
        run_scan(p, pr, kind, metric, true, s, ptile);
    }
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[1], s));
    if (kind == kScanBf16)
        launch_probe_select_approx(probe, probe_cols, probe_ld, nq, k, metric, bq, (float *)p.thr, count,
                                   bprobe ? nullptr : cand, cap, row_list, s);
    else
        launch_probe_select(probe, P, P, nq, k, metric, tau, count, cand, cap, 0, row_list, s);
    MQVS_HIP(hipGetLastError());
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[2], s));
}

// main scan in geometrically growing segments; between segments the
// threshold tightens from the candidates so far and the lists compact
// into the other buffer (keeps appends and list lengths small when the
// probe's threshold is loose, e.g. clustered data)
void FlatSearch::run_segments() {
    const int64_t align = aligned ? seg->granule : tile_rows;
    cand_alt = (Cand *)ws.cand2.get(sizeof(Cand) * (size_t)nq * cap);
    count_alt = (int *)ws.count2.get(sizeof(int) * nq);
    // (the batch probe appended nothing: the first segment also covers
    // the probe rows)
    // (a segment of fewer than kMinSegRows rows cannot fill the chip --
    // 256 tiles -- and costs a launch and a refinement: small-k searches
    // over mid-size parts, e.g. the index's coarse step, 39063 centroids
    // at k = nprobe, used to run 7 segments of 2..64 tiles)
    int64_t b = bprobe ? 0 : P, seg_rows = std::max<int64_t>({tune.first * P, align, kMinSegRows});
    int segs = 0;
    // dense gathered lists (L2 / IP) at nq <= 16: segments of at most
    // 2^19 positions in kBfRowsSmall-row tiles too (a gathered row costs
    // a list lookup before its loads; 4x the waves in flight hide it):
    // 1 % of 50M rows, nq 1: 0.420 -> 0.404 ms.  Not for cosine lists,
    // padded per chunk to whole 256-row tiles (4x the workgroups, most
    // of them padding: 1 %, nq 1 0.50 -> 0.68 ms), nor long segments
    // (L2 50 %, nq 16: 8.79 -> 9.01 ms); profiles/r05/small_tiles/main_ab.jsonl
    const bool small_main = kind == kScanBf16 && row_list && !cos && tune_int("MQVS_HI_SMALL_MAIN", 1) == 1 &&
                            scan_hi_small_tiles_ok(nq, seg->dpad);
    while (b < scan_n) {
        const int64_t e = std::min(scan_n, round_up(b + seg_rows + (segs == 0 && bprobe ? P : 0), align));
        const bool tev = timing && 2 * segs + 1 < Workspace::kSegEv;
        if (tev) MQVS_HIP(hipEventRecord(ws.seg_ev[2 * segs], s));
        const int64_t mtile = (small_main && e - b <= (int64_t)1 << 19) ? kBfRowsSmall : tile_rows;
        run_scan(p, make_range(b, e, mtile, seg->granule, aligned), kind, metric, false, s, mtile);
        if (tev) MQVS_HIP(hipEventRecord(ws.seg_ev[2 * segs + 1], s));
        if (tev) ++seg_events;
        b = e;
        seg_rows *= tune.growth;
        ++segs;
        if (b < scan_n) {
            launch_refine(cand, count, cap, nq, k, metric, kind == kScanBf16, bq, tau, (float *)p.thr, cand_alt,
                          count_alt, s);
            MQVS_HIP(hipGetLastError());
            std::swap(cand, cand_alt);
            std::swap(count, count_alt);
            p.cand = cand;
            p.cand_count = count;
        }
    }
    st.segments = segs;
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[3], s));
}

void FlatSearch::final_select() {
    if (kind == kScanBf16) {
        // survivors of the bound: up to kSortCap per query (kLargeCap with
        // the global-scratch sort for k > kSortCap)
        const int lcap = large ? kLargeCap : kSortCap;
        const int64_t rs = large ? 2 * (int64_t)kLargeCap : kSortCap;
        auto *surv = (uint32_t *)ws.surv.get(sizeof(uint32_t) * (size_t)nq * rs + sizeof(int) * nq);
        int *scnt = (int *)(surv + (size_t)nq * rs);
        uint4 *recs = large ? large : (uint4 *)ws.recs.get(sizeof(uint4) * (size_t)nq * rs);
        // (a synchronous call: the final select also stores the status words
        // into the pinned record the host reads after its wait)
        const bool fold = !async;
        launch_rerank_select(p, metric, bq, k, seg->row_offset, out.ids, out.dist, overflow, surv, scnt, recs, lcap,
                             rs, s, fold ? fl : nullptr, fold ? ws.host_flags + 16 : nullptr);
        flags_folded = fold;
    } else
        launch_final_select(cand, count, cap, nq, k, metric, seg->granule, seg->row_offset, out.ids, out.dist,
                            overflow, large, s);
    MQVS_HIP(hipGetLastError());
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[4], s));

    st.path = kind;
    st.prefilter = kind == kScanBf16 ? seg->split : 0;
    st.batch_kernel = take_batch_kernel_flag();
    st.probe_rows = P;
    st.main_rows = bprobe ? scan_n : scan_n - P;
    st.rows_scanned = scan_n;
    st.nq = nq;
    st.k = k;
    ws.pending_timing = false;
}

// no host fallback possible: leave the outcome for mqvs_async_check (or the
// caller's word)
void FlatSearch::finish_async() {
    const bool variants_matter = ords > maxv;
    launch_async_flags(overflow, status, variants_matter ? 1 : 0, a.async_word ? a.async_word : sticky_word(ws, s), s);
    MQVS_HIP(hipGetLastError());
    if (a.async_word) {
        // the survivor stats land in pinned memory, read after the
        // caller's sync (search_collect_stats)
        MQVS_HIP(hipMemcpyAsync(ws.host_flags + 16, fl, 8 * sizeof(int), hipMemcpyDeviceToHost, s));
        ws.pending_timing = timing;
        ws.pending_bf16 = kind == kScanBf16;
        ws.pending_seg_events = seg_events;
    }
    search_stats() = st;
}

void FlatSearch::finish_sync() {
    // [overflow 4][status 4] in one copy -> host_flags[0] overflow bits,
    // [1] status, [4..6] survivor / candidate stats
    // (host outputs: copied with the status words, one wait)
    ws.io.finish_begin(out, s);
    // (stored by the final select when it could; else a one-wave kernel
    // storing into the pinned words -- the runtime's device-to-host copy
    // is a 4.4 us blit kernel at the end of every search)
    if (!flags_folded) {
        launch_words_to_host(nullptr, 0, fl, 8, nullptr, ws.host_flags + 16, s);
        MQVS_HIP(hipGetLastError());
    }
    host_wait(s);
    ws.host_flags[0] = ws.host_flags[16];
    ws.host_flags[1] = ws.host_flags[20];
    ws.host_flags[4] = ws.host_flags[17];
    ws.host_flags[5] = ws.host_flags[18];
    ws.host_flags[6] = ws.host_flags[19];
    if (kind == kScanBf16) {
        st.survivors_max = ws.host_flags[4];
        st.survivors_total = (uint32_t)ws.host_flags[5];
        st.candidates_max = ws.host_flags[6];
    }
    // the fallbacks re-invoke the whole search (its stats are then the call's)
    if (const int want = check_variant_chain(ws.host_flags[1], ords, maxv)) {
        FlatArgs b = a;
        b.maxv_hint = want;
        b.formula_nq = fnq;
        search_impl(b);
        return;
    }
    if (kind == kScanBf16 && ws.host_flags[0]) {
        // the bf16 bound left too many candidates: exact fp32 path
        FlatArgs b = a;
        b.force_exact = true;
        b.maxv_hint = maxv;
        b.formula_nq = fnq;
        search_impl(b);
        search_stats().rescans += 1;
        return;
    }
    OverflowRescan r{cand, cand_alt, count, count_alt, cap, nq, k, metric, tau, overflow, seg->granule,
                     seg->row_offset, out.ids, out.dist, large, scan_n, aligned ? seg->granule : tile_rows};
    st.rescans = rescan_on_overflow(ws, r, s, [&](int64_t b, int64_t e, Cand *to, int *to_count) {
        p.cand = to;
        p.cand_count = to_count;
        run_scan(p, make_range(b, e, tile_rows, seg->granule, aligned), kind, metric, false, s);
    });
    if (st.rescans)
        ws.io.finish(out, s);
    else
        ws.io.finish_end(out);
    if (timing) read_search_times(ws, st, seg_events);
    search_stats() = st;
}

// validate, split into query sub-batches where one batch's scratch would not
// fit, and run the stages
static void search_impl(const FlatArgs &a) {
    mqvs_segment *seg = a.seg;
    const int nq = a.nq, k = a.k, metric = a.metric;
    const int fnq = a.formula_nq > 0 ? a.formula_nq : nq;
    check_search_args(seg, "segment",
                      seg && seg->binary ? "binary (FixedString) segment: search it with mqvs_search_binary" : nullptr,
                      nq, k, a.queries, a.out_ids, a.out_dist);
    const bool cos = metric == MQVS_METRIC_COSINE;
    if (metric != MQVS_METRIC_L2 && metric != MQVS_METRIC_IP && !cos && metric != kMetricIpRaw)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Float32 Vector");
    if (cos != (seg->metric == MQVS_METRIC_COSINE))
        fail(MQVS_ERR_LOGICAL, "segment was prepared for a different metric (cosine segments are "
                               "normalised in HBM and serve only cosine searches)");
    search_stats() = mqvs_search_stats{};
    if (nq == 0 || k == 0) return;
    auto sub_batches = [&](int64_t qb) {
        for_query_batches(nq, qb, [&](int q0, int m) {
            FlatArgs b = a;
            b.queries = a.queries + (size_t)q0 * seg->d;
            b.nq = m;
            b.out_ids = a.out_ids + (size_t)q0 * k;
            b.out_dist = a.out_dist + (size_t)q0 * k;
            b.formula_nq = fnq;
            search_impl(b);
        });
    };
    if (k > kSortCap) {
        // large k: query sub-batches (queries are independent searches)
        const int qb = large_k_batch(seg->n, k);
        if (nq > qb) return sub_batches(qb);
    }
    if (a.maxv_hint > kMaxVariants) {
        // a grown cosine variant table (chains that did not repeat within the
        // default table): its fp32 variants and their bf16 plane are
        // maxv x (4 qstride + 2 dpad) bytes per query -- query sub-batches
        // keep them within the scratch budget (same formula, same bits)
        const int64_t per_q = (int64_t)a.maxv_hint * (round_up(seg->d, 32) * 4 + round_up(seg->d, kBfK) * 2);
        const int64_t qb = std::max<int64_t>(1, (int64_t)scratch_budget() / per_q);
        if (nq > qb) return sub_batches(qb);
    }

    DeviceGuard guard(seg->device);
    Workspace &ws = workspace(seg->device);
    WsCall ws_call(ws);
    hipStream_t s = a.user_stream ? a.user_stream : ws.stream;
    ws.last = s;
    FlatSearch(a, ws, s).run();
}

void read_search_times(Workspace &ws, mqvs_search_stats &st, int seg_events) {
    float a = 0, b = 0, c = 0, e = 0, f = 0;
    MQVS_HIP(hipEventElapsedTime(&a, ws.ev[5], ws.ev[1]));
    MQVS_HIP(hipEventElapsedTime(&b, ws.ev[1], ws.ev[2]));
    MQVS_HIP(hipEventElapsedTime(&c, ws.ev[2], ws.ev[3]));
    MQVS_HIP(hipEventElapsedTime(&e, ws.ev[3], ws.ev[4]));
    MQVS_HIP(hipEventElapsedTime(&f, ws.ev[0], ws.ev[4]));
    st.probe_ms = a;
    st.probe_select_ms = b;
    // main_ms: the scan kernels only; refine_ms: the refinements between
    float scan = 0.f;
    const int ns = std::min(seg_events, Workspace::kSegEv / 2);
    for (int i = 0; i < ns; ++i) {
        float x = 0.f;
        MQVS_HIP(hipEventElapsedTime(&x, ws.seg_ev[2 * i], ws.seg_ev[2 * i + 1]));
        scan += x;
    }
    st.main_ms = ns > 0 ? scan : c;
    st.refine_ms = ns > 0 ? c - scan : 0.0;
    st.final_ms = e;
    st.total_ms = f;
}

// the stats of this thread's last search_segment_async on `device`, once the
// caller has synchronised its stream
void search_collect_stats(int device) {
    Workspace &ws = workspace(device);
    WsCall ws_call(ws);
    mqvs_search_stats &st = search_stats();
    if (ws.pending_bf16) {
        st.survivors_max = ws.host_flags[17];
        st.survivors_total = (uint32_t)ws.host_flags[18];
        st.candidates_max = ws.host_flags[19];
    }
    if (ws.pending_timing) read_search_times(ws, st, ws.pending_seg_events);
    ws.pending_timing = ws.pending_bf16 = false;
}

// the FLAT search of a segment (the C entry points, index.hip)
void search_internal(mqvs_segment *seg, const float *queries, int nq, int k, int metric, const uint8_t *filter,
                     const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t stream,
                     int64_t ord_base) {
    FlatArgs a{seg, queries, nq, k, metric, filter, exists, out_ids, out_dist, flags, stream};
    a.ord_base = ord_base;
    search_impl(a);
}

// the search for other translation units (sharded.hip): device pointers,
// caller stream, explicit chunk-ordinal base
void search_segment(mqvs_segment *seg, const float *queries, int nq, int k, int metric, const uint8_t *filter,
                    const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t stream,
                    int64_t ord_base) {
    search_internal(seg, queries, nq, k, metric, filter, exists, out_ids, out_dist, flags | MQVS_F_DEVICE_PTRS, stream,
                    ord_base);
}

// the same without any host sync: fallback flags OR-ed into *flag_word
// (bit 0 candidate overflow, bit 1 cosine variant table too short), stats
// collected by search_collect_stats after the caller's sync
void search_segment_async(mqvs_segment *seg, const float *queries, int nq, int k, int metric, const uint8_t *filter,
                          const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags,
                          hipStream_t stream, int64_t ord_base, int *flag_word) {
    FlatArgs a{seg,      queries, nq, k, metric, filter, exists, out_ids,
               out_dist, flags | MQVS_F_DEVICE_PTRS | MQVS_F_ASYNC, stream};
    a.ord_base = ord_base;
    a.async_word = flag_word;
    search_impl(a);
}

// Exact re-rank of caller-given candidate rows (computeTopDistanceSubset
// contract, VIWithDataPart.cpp:838-856): the distance formula and cosine
// query variant mqvs_search uses for the same batch size, then top-k by the
// reference key.  Rows < 0, >= n or deleted (row_exists) are skipped; the
// candidate list of a query is expected to hold distinct rows.
static void rerank_impl(mqvs_segment *seg, const float *queries, int nq, const int64_t *cand,
                        int ncand, int k, int metric, const uint8_t *exists, int64_t *out_ids,
                        float *out_dist, uint32_t flags, hipStream_t user_stream, int formula_nq = 0) {
    const int fnq = formula_nq > 0 ? formula_nq : nq;  // (see FlatArgs)
    if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
    if (seg->binary) fail(MQVS_ERR_NOT_IMPLEMENTED, "computeTopDistanceSubset is for Float32 vectors");
    if (nq < 0 || k < 0 || ncand < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "nq, k and ncand must be non-negative");
    const bool cos = metric == MQVS_METRIC_COSINE;
    if (metric != MQVS_METRIC_L2 && metric != MQVS_METRIC_IP && !cos)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Float32 Vector");
    if (cos != (seg->metric == MQVS_METRIC_COSINE))
        fail(MQVS_ERR_LOGICAL, "segment was prepared for a different metric");
    if (k > kMaxK || ncand > kLargeCap)
        fail(MQVS_ERR_BAD_ARGUMENTS, "k must not exceed " + std::to_string(kMaxK) + " and ncand " +
                                         std::to_string(kLargeCap));
    if (nq > 0 && k > 0 && (!queries || !out_ids || !out_dist || (ncand > 0 && !cand)))
        fail(MQVS_ERR_BAD_ARGUMENTS, "null query, candidate or output pointer");
    search_stats() = mqvs_search_stats{};
    if (nq == 0 || k == 0) return;
    // more candidates than the LDS sort holds: each query's records are sorted
    // through 2 ncand records of global scratch, in query sub-batches of <= 1 GB
    const bool large = ncand > kSortCap;
    if (large) {
        const int qb = (int)std::max<int64_t>(1, (int64_t)scratch_budget() / 16 / (2 * (int64_t)ncand));
        if (nq > qb) {
            for_query_batches(nq, qb, [&](int q0, int m) {
                rerank_impl(seg, queries + (size_t)q0 * seg->d, m, cand + (size_t)q0 * ncand, ncand, k, metric,
                            exists, out_ids + (size_t)q0 * k, out_dist + (size_t)q0 * k, flags, user_stream, fnq);
            });
            return;
        }
    }

    DeviceGuard guard(seg->device);
    Workspace &ws = workspace(seg->device);
    WsCall ws_call(ws);
    hipStream_t s = user_stream ? (hipStream_t)user_stream : ws.stream;
    ws.last = s;
    const bool dev = flags & MQVS_F_DEVICE_PTRS;
    const bool async = dev && (flags & MQVS_F_ASYNC);
    const int d = seg->d;
    // (copies queued in this order: queries, candidate rows, row_exists)
    const size_t qbytes = sizeof(float) * (size_t)nq * d;
    const auto *dq = (const float *)ws.io.in(queries, qbytes, nullptr, nullptr, 0, dev, s).queries;
    const auto *dc = dev ? cand : (const int64_t *)ws.io.in_list(cand, sizeof(int64_t) * (size_t)nq * ncand, s);
    const uint8_t *dexists = ws.io.in(nullptr, 0, nullptr, exists, (seg->n + 7) / 8, dev, s).exists;
    const CallIO::Out out = ws.io.out((size_t)nq * k, dev, out_ids, out_dist);
    const bool blas = fnq >= kBlasThreshold;
    const int64_t ords = seg->row_offset / seg->granule + (seg->n + seg->granule - 1) / seg->granule;
    float *qvars = nullptr, *qnorms = nullptr;
    int *qmu = nullptr, *qlam = nullptr, *status = nullptr;
    const int maxv = prep_variants(ws, dq, nq, d, cos, blas && metric == MQVS_METRIC_L2, ords, !async, qvars, qnorms,
                                   qmu, qlam, status, s);

    ScanParams p{};
    p.rows = seg->rows;
    p.row_norms = seg->norms;
    p.n = seg->n;
    p.d = d;
    p.nq = nq;
    p.qvars = qvars;
    p.qnorms = qnorms;
    p.qmu = qmu;
    p.qlam = qlam;
    p.maxv = maxv;
    p.blas_nq = fnq;
    p.chunk_rows = seg->granule;
    p.chunk_ord = seg->chunk_ord;
    p.ord_base = (int)(seg->row_offset / seg->granule);
    p.exists = dexists;
    p.nonempty = seg->nonempty_bits;
    uint4 *scratch = large ? (uint4 *)ws.large.get(sizeof(uint4) * 2 * (size_t)ncand * nq) : nullptr;
    launch_rerank_ids(p, metric, dc, ncand, k, seg->row_offset, out.ids, out.dist, scratch, s);
    MQVS_HIP(hipGetLastError());
    if (async) {
        launch_async_flags(nullptr, status, ords > maxv ? 1 : 0, sticky_word(ws, s), s);
        MQVS_HIP(hipGetLastError());
        return;
    }
    ws.io.finish_begin(out, s);
    MQVS_HIP(hipMemcpyAsync(ws.host_flags, status, sizeof(int), hipMemcpyDeviceToHost, s));
    host_wait(s);
    // (prep_variants has grown the table where it could: nothing to retry with)
    (void)check_variant_chain(ws.host_flags[0], ords, maxv, false);
    ws.io.finish_end(out);
}

void rerank_flat(mqvs_segment *seg, const float *queries, int nq, const int64_t *cand, int ncand, int k, int metric,
                 const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t stream) {
    rerank_impl(seg, queries, nq, cand, ncand, k, metric, exists, out_ids, out_dist, flags, stream);
}

}  // namespace mqvs
