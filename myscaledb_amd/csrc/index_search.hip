// index_search.hip -- the float index search of libmqvs (mqvs_index_search,
// mqvs_index_probes; the build: index_build.hip, the C glue: index.hip), and
// what it shares with the binary index search (index_search_binary.hip): the
// nprobe resolution and the stats read.
//
// Search:
//   coarse   FLAT search of the queries against the centroid segment, k =
//            nprobe (L2 for L2 parts, raw inner product for IP and cosine)
//   plan     (query, list) pairs grouped by list into 16-query work items
//   scan     bf16 MFMA over each probed list (kernels_ivf_scan.hip); an index built
//            with plane=fp8 keeps e4m3fn codes there, widened in registers
//   select   num_reorder best approximate values per query
//   re-rank  exact fp32 distances of those rows (k_rerank_ids: the formula
//            and cosine query variant of mqvs_search / mqvs_rerank), top-k by
//            the reference order key
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "index_internal.h"

namespace mqvs {

// ---- one list pass ----------------------------------------------------------

// A list layout as a pass scans it: the index's lists (fine) or the coarse
// quantizer's centroid chunks (coarse).  A view: the arrays are the index's.
struct ListLayout {
    const uint16_t *plane = nullptr;  // bf16 rows in list order (null for an fp8 plane), or
    const uint8_t *plane8 = nullptr;  // the e4m3fn codes and
    const int16_t *pscale = nullptr;  // each position's scale exponent
    const int32_t *perm = nullptr;
    const float *pnorm = nullptr;
    const int64_t *list_off = nullptr;
    int64_t nlist = 0, npos = 0, max_list = 0, dpad = 0;
    int esize = 2;  // bytes per plane element
};

static ListLayout fine_layout(const mqvs_index *ix) {
    ListLayout l;
    if (ix->plane_fmt == MQVS_INDEX_PLANE_FP8) {
        l.plane8 = ix->plane8;
        l.pscale = ix->pscale;
        l.esize = 1;
    } else {
        l.plane = ix->plane;
    }
    l.perm = ix->perm;
    l.pnorm = ix->pnorm;
    l.list_off = ix->list_off;
    l.nlist = ix->nlist;
    l.npos = ix->npos;
    l.max_list = ix->max_list;
    l.dpad = ix->dpad;
    return l;
}

static ListLayout coarse_layout(const mqvs_index *ix) {
    ListLayout l;
    l.plane = ix->cplane;
    l.perm = ix->cperm;
    l.pnorm = ix->cpnorm;
    l.list_off = ix->clist_off;
    l.nlist = ix->cnl;
    l.npos = ix->cnpos;
    l.max_list = ix->cmax;
    l.dpad = ix->dpad;
    return l;
}

// What one pass is asked for.  probes[nq][nprobe] are list ids; out_rows: the
// R best rows per query by the approximate distance (+ id_offset; with
// out_approx, ids and approximate distances for a first-stage result; out_raw:
// the R scan values, for the re-rank's pruning).
struct ListArgs {
    int metric = 0;
    hipStream_t s = nullptr;
    // queries: bf16 values (for an fp8 plane: the queries' scaled codes as
    // bf16 values, with their scale exponents in qexp), |q|^2
    const uint16_t *qhi = nullptr;
    const float *qnorm = nullptr;
    const int16_t *qexp = nullptr;
    int nq = 0;
    const int64_t *probes = nullptr;
    int nprobe = 0;
    const uint8_t *filter = nullptr, *exists = nullptr;
    int R = 0;
    int64_t *out_rows = nullptr;
    int64_t id_offset = 0;
    float *out_approx = nullptr, *out_raw = nullptr;
    hipEvent_t *ev = nullptr;       // (optional) events 2..4 after plan, scan and select
    bool dense = false;             // every query probes every list, probe r = list r (probes unused)
    int64_t *pair_stats = nullptr;  // [nq][4] words (null: no pair mode)
};

// the stats words of a pass; per_query: they are pair mode's per-query rows
struct ListStats {
    int64_t *words;
    bool per_query;
};

// the work item shape of a pass: queries per item (p.qg) and list positions
// per item (p.chunk)
static void list_item_shape(IvfParams &p, const ListLayout &l, const ListArgs &a) {
    const int64_t E = (int64_t)a.nq * a.nprobe;
    // 32-query work items when lists are probed by many queries (each A
    // fragment then feeds two MFMAs)
    // (64-query items, QB = 4, measured slower on the dense coarse pass at
    // d = 768: its 99 KiB LDS tile leaves one workgroup per CU)
    // Lists probed by very many queries (IVF-hostile data at large nprobe):
    // 64-query items halve the list re-reads again (10M x 768, nq 1000,
    // nprobe 512 = 51 queries per list: 14.4 -> 12.3 ms; at 13 per list
    // they are slower, tools/index_qg_ab.py).
    p.qg = (!a.dense && E >= 40 * l.nlist) ? 64 : (a.dense || E >= 24 * l.nlist) ? 32 : 16;
    if (const char *e = tune_env("MQVS_IVF_QG")) {  // A/B knob (tools/ab_split.py style)
        const int v = std::atoi(e);
        if (!a.dense && (v == 16 || v == 32 || v == 64)) p.qg = v;
    }
    // wide rows: the largest of that size and its smaller siblings whose query
    // tile fits a workgroup's LDS (64 up to dpad 1216, 32 up to 2496, 16 up to
    // 5056 with 160 KiB; the dense plan groups by whatever p.qg is).  The
    // build refuses wider rows, so something fits.
    p.qg = ivf_fit_qg(p.qg, l.dpad, device_lds_bytes());
    // (p.qg sizes the work items below; the build's own check keeps this from happening)
    if (p.qg == 0) fail(MQVS_ERR_LOGICAL, "list scan: no query tile fits the workgroup's LDS");
    // work items = sum over probed lists of groups x 512-position slices
    // list positions per work item (a multiple of 64): 8 x the item's queries,
    // so the query tile stays a fixed share of the bytes an item reads (round
    // 5: 128 for 16-query items, 512 before -- the item setup's chain of
    // dependent loads was a large part of a 256-position list's scan; mode 3
    // nprobe 1 scan 0.139 -> 0.117 ms, profiles/r05/index_scan/)
    p.chunk = a.dense ? kIvfChunk : std::max(64, tune_int("MQVS_IVF_CHUNK", 8 * p.qg) / 64 * 64);
}

// One list pass: plan + bf16 MFMA scan + select of the queries over a list
// layout.  Few pairs per list take pair mode (no plan; the select writes each
// query's stats to pair_stats).
static ListStats list_pass(ListBufs &b, const ListLayout &l, const ListArgs &a) {
    const int nq = a.nq, nprobe = a.nprobe;
    const int64_t nlist = l.nlist;
    hipStream_t s = a.s;
    const int64_t E = (int64_t)nq * nprobe;
    IvfParams p{};
    p.plane = l.plane;
    p.perm = l.perm;
    p.pnorm = l.pnorm;
    p.list_off = l.list_off;
    p.nlist = (int)nlist;
    p.dpad = l.dpad;
    p.nq = nq;
    p.nprobe = nprobe;
    p.probes = a.probes;
    p.q_hi = a.qhi;
    p.qnorm = a.qnorm;
    p.filter = a.filter;
    p.exists = a.exists;
    p.esize = l.esize;
    p.plane8 = l.plane8;
    p.pscale = l.pscale;
    p.qexp = a.qexp;
    p.lcount = (int *)b.lcount.get(sizeof(int) * nlist);
    p.lfill = (int *)b.lfill.get(sizeof(int) * nlist);
    p.lstart = (int64_t *)b.lstart.get(sizeof(int64_t) * nlist);
    p.lq = (int *)b.lq.get(sizeof(int) * E);
    list_item_shape(p, l, a);
    // Pair mode: with about one query per probed list the plan groups
    // nothing; it only orders the pairs (six launches over every list: ~43 us
    // at 39063 lists, nq 1000, nprobe 1).  Instead every (pair, slice) is a
    // work item of its own, each query's region a fixed stride.  Lists probed
    // by several queries are then read once per query (mode 2 at nprobe 1:
    // ~10 % of its list bytes twice).
    const bool pairs = a.pair_stats && !a.dense && p.qg == 16 && 16 * E <= nlist && l.max_list > 0 &&
                       (double)nq * nprobe * (l.max_list / p.chunk + 1) < 2e9 && tune_int("MQVS_IVF_PAIR", 1) == 1;
    IvfRegions rg;
    if (pairs) {
        p.pair_stride = (int64_t)nprobe * l.max_list;
        p.pair_nch = (int)((l.max_list + p.chunk - 1) / p.chunk);
        p.stats = a.pair_stats;
        p.cand = (Cand *)b.cand.get(sizeof(Cand) * (size_t)std::max<int64_t>((int64_t)nq * p.pair_stride, 1));
        rg.stride = p.pair_stride;
        rg.nprobe = nprobe;
        rg.nlist = (int)nlist;
        rg.chunk = p.chunk;
        rg.dpad = l.dpad;
        rg.esize = p.esize;
        rg.probes = a.probes;
        rg.list_off = l.list_off;
        rg.stats = a.pair_stats;
    } else {
        const int64_t max_items = (E / p.qg + std::min<int64_t>(E, nlist)) * (l.max_list / p.chunk + 1);
        p.item_list = (int *)b.items.get(sizeof(int) * max_items);
        p.item_grp = (int *)b.grp.get(sizeof(int) * max_items);
        p.item_chk = (int *)b.chk.get(sizeof(int) * max_items);
        p.nitems = (int *)b.nitems.get(sizeof(int) * 4);
        p.qbase = (int64_t *)b.qbase.get(sizeof(int64_t) * E);
        p.qstart = (int64_t *)b.qstart.get(sizeof(int64_t) * (nq + 1));
        // a query's region is at most min(nprobe * longest list, every position)
        const int64_t cap = (int64_t)nq * std::min<int64_t>((int64_t)nprobe * l.max_list, l.npos);
        p.cand = (Cand *)b.cand.get(sizeof(Cand) * (size_t)std::max<int64_t>(cap, 1));
        const int64_t plan_wgs = (nlist + 4095) / 4096;  // k_plan_lists_* workgroups (>= 4096 lists each)
        p.stats = (int64_t *)b.stats.get(sizeof(int64_t) * (8 + 3 * plan_wgs));
        p.bsum = p.stats + 8;
        if (a.dense)
            launch_ivf_plan_dense(p, l.npos, s);
        else
            launch_ivf_plan(p, s);
        MQVS_HIP(hipGetLastError());
        rg.qstart = p.qstart;
    }
    if (a.ev) MQVS_HIP(hipEventRecord(a.ev[2], s));
    // (a workgroup per work item up to 4096: ~2900 items at nq 1000, nprobe 1)
    launch_ivf_scan(p, a.metric, a.dense ? 1024 : tune_int("MQVS_IVF_GRID", 4096), s);
    MQVS_HIP(hipGetLastError());
    if (a.ev) MQVS_HIP(hipEventRecord(a.ev[3], s));
    const int64_t expect =
        a.dense ? l.npos : (int64_t)((double)nprobe * l.npos / std::max<int64_t>(nlist, 1) * 1.5);
    // R above kSortCap: the select sorts through 2 R records of scratch per query
    uint4 *gscr = a.R > kSortCap ? (uint4 *)b.large.get(sizeof(uint4) * 2 * (size_t)a.R * nq) : nullptr;
    launch_ivf_select(p.cand, rg, nq, a.R, a.metric, a.out_rows, a.id_offset, a.out_approx, expect, s, gscr, a.out_raw);
    MQVS_HIP(hipGetLastError());
    if (a.ev) MQVS_HIP(hipEventRecord(a.ev[4], s));
    return ListStats{p.stats, pairs};
}

// ---- the search of one query batch --------------------------------------------
// Stages over the search's state, as FlatSearch (search.hip): run() queues
// them in order on one stream; every stage reads what earlier ones left in
// the members, and the buffers are the workspace's.  The parameters are
// resolved, and the workspace admitted, by search_index_impl below.
struct IndexSearch {
    // ---- call inputs
    mqvs_index *const ix;
    mqvs_segment *const seg;
    IndexWorkspace &ws;
    const hipStream_t s;
    const float *const queries;
    const int nq, k;
    const uint8_t *const filter, *const exists;
    int64_t *const out_ids;
    float *const out_dist;
    const uint32_t flags;
    const int fnq;         // the call's batch size, which selects the exact re-rank's distance formula
    const int nprobe, R;   // as resolved from the search parameters
    // the ordinal of the segment's first searched chunk (cosine: selects the
    // re-rank's query variant per row): the caller's (a row-range shard whose
    // lower ranks' searched chunks were counted), else row_offset / granule
    const int64_t ord_base;
    int *const async_word;  // ASYNC: where the outcome flags go (null: the thread's sticky word)
    // mqvs_index_probes: the coarse step's probes[nq][nprobe] are copied
    // there and the search ends
    int64_t *const probes_out;
    // ---- derived constants
    const int d;
    const bool dev, async, cos, first_stage, fp8;
    // per-stage timing events only when asked (MQVS_F_TIMING / mqvs_set_timing:
    // ev[0..4]); ev[5] ends every search (the workspace trim waits on it)
    const bool tev;
    // Cosine: only variant 0 is needed before the exact re-rank (coarse step,
    // list scan), so the rest of the chain -- a sequential fp32 sum per
    // normalisation, up to kMaxVariants of them: 60-130 us at nq 1000 -- runs
    // on the side stream meanwhile and is joined before the re-rank.
    const bool split;
    const int64_t ords;  // chunk ordinals the part's searches reach
    const int maxv;      // variants per query in the table
    const int64_t qstride;
    // ---- device pointers
    const float *dq = nullptr;
    const uint8_t *dfilter = nullptr, *dexists = nullptr;
    CallIO::Out out{};
    float *qvars = nullptr, *qnorms = nullptr;
    int *qmu = nullptr, *qlam = nullptr;
    int *status = nullptr;                // [status 4 ints][pick overflow queries, candidates re-ranked: 2 x u64]
    unsigned long long *istat = nullptr;  // the two u64 of it
    int64_t *pstats = nullptr;            // the fine pass's per-query stats in pair mode
    uint16_t *qhi = nullptr;              // variant 0 as bf16
    uint16_t *q8 = nullptr;               // fp8 plane: variant 0's scaled codes as bf16 values,
    int16_t *q8exp = nullptr;             //   their scale exponents
    float *q8rec = nullptr;               //   and norm records
    int64_t *probes = nullptr;
    float *qrec0 = nullptr;  // variant 0's norm records (the pick's bound; the re-rank pruning's)
    bool prune = false;
    float *craw = nullptr, *ibq = nullptr;
    float *qdelta = nullptr;  // cosine, pruned re-rank: the chain's variant spread (k_query_prep phase 2)
    int64_t *crow = nullptr;  // the candidates of the re-rank
    ListStats fine_stats{nullptr, false};
    // the side stream's variant chain is joined into s on EVERY exit after it
    // forks (an exception between fork and the re-rank's wait included), so
    // the next search on this thread -- whose prep rewrites qvars and status
    // on s -- and a trimmer waiting for s's completion see it finished
    struct JoinGuard {
        hipStream_t s;
        hipEvent_t ev;
        bool on = false;
        ~JoinGuard() {
            if (on) (void)hipStreamWaitEvent(s, ev, 0);
        }
    } join_guard;
    // ---- stats
    mqvs_index_search_stats st;

    IndexSearch(mqvs_index *index, IndexWorkspace &w, hipStream_t stream, const float *q, int nq_, int k_,
                const uint8_t *filter_, const uint8_t *exists_, int64_t *ids, float *dist, uint32_t flags_, int fnq_,
                int nprobe_, int R_, int maxv_hint, int64_t ord_base_, int *async_word_,
                int64_t *probes_out_, const mqvs_index_search_stats &header)
        : ix(index), seg(index->seg), ws(w), s(stream), queries(q), nq(nq_), k(k_), filter(filter_), exists(exists_),
          out_ids(ids), out_dist(dist), flags(flags_), fnq(fnq_), nprobe(nprobe_), R(R_),
          ord_base(ord_base_ >= 0 ? ord_base_ : index->seg->row_offset / index->seg->granule),
          async_word(async_word_), probes_out(probes_out_), d(seg->d),
          dev(flags_ & MQVS_F_DEVICE_PTRS), async(dev && (flags_ & MQVS_F_ASYNC)),
          cos(index->metric == MQVS_METRIC_COSINE), first_stage(flags_ & MQVS_F_FIRST_STAGE),
          fp8(index->plane_fmt == MQVS_INDEX_PLANE_FP8), tev(timing_on(flags_)), split(cos && !first_stage),
          ords(ord_base + (seg->n + seg->granule - 1) / seg->granule),
          maxv(cos ? (maxv_hint > 0 ? maxv_hint : kMaxVariants) : 1), qstride(round_up(d, 32)),
          join_guard{stream, w.join}, st(header) {}

    void stage_inputs();
    void prep_queries();
    void quantise_queries();
    void coarse();
    void coarse_every_list();
    bool coarse_pick();
    void coarse_flat();
    void coarse_list_pass();
    void probes_only();
    void prune_bound();
    void fork_chain();
    void fine();
    void rerank();
    void queue_stats();
    void finish_async();
    int finish_sync();

    // 0, or (a cosine variant chain that did not repeat within the table) the
    // table size to run the search again with
    int run() {
        stage_inputs();
        prep_queries();
        quantise_queries();
        coarse();
        if (probes_out) {
            probes_only();
            return 0;
        }
        prune_bound();
        if (split) fork_chain();
        fine();
        if (!first_stage) rerank();
        MQVS_HIP(hipEventRecord(ws.ev[5], s));
        // decoupled part: results in the new part's row ids (VIWithDataPart.cpp:938-943)
        if (dev && ix->row_ids_map) launch_map_ids(out.ids, (int64_t)nq * k, ix->row_ids_map, s);
        if (async) {
            finish_async();
            return 0;
        }
        return finish_sync();
    }
};

void IndexSearch::stage_inputs() {
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[0], s));
    const CallIO::In in = ws.io.in(queries, sizeof(float) * (size_t)nq * d, filter, exists, (seg->n + 7) / 8, dev, s);
    dq = (const float *)in.queries;
    dfilter = in.filter;
    dexists = in.exists;
    out = ws.io.out((size_t)nq * k, dev, out_ids, out_dist);
}

// ---- query prep: cosine re-normalisation variants (the re-rank uses the
// row's chunk variant, as mqvs_search does), |q|^2.  The variant table
// starts at kMaxVariants per query with no host round trip; a chain that
// does not repeat within it on a part of more chunk ordinals (rare:
// small-integer data) is caught from the status word read at the end, and
// the search re-runs with the larger table (as mqvs_search does).  The
// table is not cleared: every variant a reader can select (ordinal < mu +
// lambda, or < maxv when the chain did not repeat) is written by the prep.
void IndexSearch::prep_queries() {
    qvars = (float *)ws.qvars.get(sizeof(float) * (size_t)nq * maxv * qstride);
    qnorms = (float *)ws.qnorms.get(sizeof(float) * nq);
    qmu = (int *)ws.qmu.get(sizeof(int) * nq);
    qlam = (int *)ws.qlam.get(sizeof(int) * nq);
    status = (int *)ws.status.get(sizeof(int) * 8);
    launch_fill2(reinterpret_cast<uint32_t *>(status), 8, 0u, nullptr, 0, 0u, s);
    istat = reinterpret_cast<unsigned long long *>(status + 4);
    pstats = (int64_t *)ws.pstats.get(sizeof(int64_t) * 4 * (size_t)nq);
    launch_query_prep(dq, nq, d, cos ? MQVS_METRIC_COSINE : MQVS_METRIC_L2, ix->metric == MQVS_METRIC_L2, qvars, maxv,
                      qnorms, qmu, qlam, status, s, split ? 1 : 0);
    MQVS_HIP(hipGetLastError());
}

// variant 0 of every query in the list plane's format: bf16, or for an fp8
// plane the query's own e4m3fn codes (as the bf16 values the scan's MFMA
// takes) with its scale exponent and norm records (the bf16 rounding is
// then made only if the coarse step takes the centroid list pass)
void IndexSearch::quantise_queries() {
    qhi = (uint16_t *)ws.qhi.get(sizeof(uint16_t) * (size_t)nq * ix->dpad);
    if (fp8) {
        q8 = (uint16_t *)ws.q8.get(sizeof(uint16_t) * (size_t)nq * ix->dpad);
        q8exp = (int16_t *)ws.q8exp.get(sizeof(int16_t) * (size_t)nq);
        q8rec = (float *)ws.q8rec.get(sizeof(float) * kMxRec * (size_t)nq);
        launch_to_fp8(qvars, (int64_t)maxv * qstride, d, nullptr, nq, ix->dpad, nullptr, q8, q8exp, nullptr, nullptr,
                      q8rec, nullptr, s);
    } else {
        launch_to_bf16(qvars, nq, d, (int64_t)maxv * qstride, qhi, ix->dpad, s);
    }
    MQVS_HIP(hipGetLastError());
}

// ---- coarse: the nprobe nearest centroids, by one of four forms
// many lists: the FLAT batch search of the centroid segment (exact
// top-nprobe; ranking by the raw inner product for IP and cosine parts):
// 65536 lists, nq 1000: 1.26 -> 0.67 ms; few lists: the list pass over
// the centroid chunks (10000 lists: 0.28 ms vs 0.50, the FLAT path's
// fixed stages dominate; profiles/r03/index)
// Default (nprobe <= 64 and the centroid plane present): the batch kernel
// scores every (query, centroid) on bf16 and keeps the best of each
// 8-centroid group; the nprobe best groups per query (and any other
// group the bf16 bound cannot rule out) then get exact fp32 values and
// the nprobe best of those are the probes (k_coarse_pick).  65536 or 39063 lists at nq 1000: one batch-kernel
// launch and one pick instead of mqvs_search's whole pipeline.
void IndexSearch::coarse() {
    probes = (int64_t *)ws.probes.get(sizeof(int64_t) * (size_t)nq * nprobe);
    const int cmode = tune_int("MQVS_IVF_COARSE", 2);
    const bool pick_ok = cmode == 2 && nprobe <= kCoarsePickMaxT && ix->cent && ix->cent->rows_hi && ix->cent->rows;
    if (nprobe >= ix->nlist) {
        coarse_every_list();
    } else if (!(pick_ok && coarse_pick())) {
        if (tune_int("MQVS_IVF_COARSE", ix->nlist > kCoarseFlatLists ? 1 : 0) == 1)
            coarse_flat();
        else
            coarse_list_pass();
    }
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[1], s));
}

// every list is probed: nothing to rank, and nothing to lose -- the
// ranked forms never pick a centroid whose score is NaN (a NaN or
// infinite query; a centroid of a list that holds infinite rows)
void IndexSearch::coarse_every_list() {
    launch_iota_probes(probes, nq, nprobe, s);
    MQVS_HIP(hipGetLastError());
}

// the batch kernel and the pick; false: the batch kernel does not take this
// shape (nothing but variant 0's records is queued then)
bool IndexSearch::coarse_pick() {
    mqvs_segment *cs = ix->cent;
    const int64_t vpad = round_up(nq, 16);
    auto *cq = (uint16_t *)ws.cqhi.get(sizeof(uint16_t) * (size_t)vpad * cs->dpad);
    // (variant 0 of every query: the raw query, or the normalised one for
    // cosine -- centroids of cosine parts are normalised: same ranking as
    // the raw inner product)
    // (with the variants' norm records: the pick's bf16 bound)
    float *crec = (float *)ws.crec.get(sizeof(float) * kMxRec * (size_t)nq);
    launch_to_hi(qvars, nq, d, (int64_t)maxv * qstride, cs->dpad, 1, vpad, cq, crec, nullptr, s);
    qrec0 = crec;
    MQVS_HIP(hipGetLastError());
    ScanParams cp{};
    cp.rows_hi = cs->rows_hi;
    cp.row_norms = cs->norms;
    cp.n = cs->n;
    cp.d = d;
    cp.dpad = cs->dpad;
    cp.nq = nq;
    cp.q_hi = cq;
    cp.q_vpad = vpad;
    cp.maxv = 1;
    cp.qnorms = qnorms;
    cp.chunk_rows = cs->granule;
    cp.row_begin = 0;
    cp.row_end = cs->n;
    cp.tile_rows = 256;
    cp.tiles = (cs->n + 255) / 256;
    cp.tiles_per_chunk = 0;
    // groups of 8 centroids: 32 per 256-row tile
    const int64_t gld = round_up(32 * cp.tiles, 4);
    cp.p4_gmax = (float *)ws.gmax.get(sizeof(float) * (size_t)nq * gld);
    cp.p4_gld = gld;
    if (!launch_scan_p4_groups(cp, ix->coarse_metric, s)) return false;
    MQVS_HIP(hipGetLastError());
    // each query's bound on |bf16 group value - exact| (the direct
    // formula's rounding terms: the larger of the two)
    float *cbq = (float *)ws.cbq.get(sizeof(float) * (size_t)nq);
    ScanParams bp = cp;
    bp.blas_nq = 1;
    launch_query_bound(bp, ix->coarse_metric, cs->ynorm_max, crec, cs->ynorm_max + 4, cbq, nullptr, s);
    MQVS_HIP(hipGetLastError());
    // (core groups of the pick: nprobe; any count keeps the probes exact,
    // and more of them only score more centroids exactly,
    // profiles/r05/pick/core_t_ab.jsonl)
    launch_coarse_pick(cp.p4_gmax, gld, 32 * cp.tiles, nprobe, nprobe, ix->coarse_metric, qvars,
                       (int64_t)maxv * qstride, cs->rows, cs->norms, cs->n, d, cbq, qnorms, 3, nq, probes, istat, s);
    MQVS_HIP(hipGetLastError());
    return true;
}

void IndexSearch::coarse_flat() {
    float *pd = (float *)ws.pdist.get(sizeof(float) * (size_t)nq * nprobe);
    if (async && async_word) {
        // (the nested search's candidate overflow is the caller's to see too)
        search_segment_async(ix->cent, dq, nq, nprobe, ix->coarse_metric, nullptr, nullptr, probes, pd, 0, s, -1,
                             async_word);
        return;
    }
    search_internal(ix->cent, dq, nq, nprobe, ix->coarse_metric, nullptr, nullptr, probes, pd,
                    MQVS_F_DEVICE_PTRS | (flags & MQVS_F_ASYNC), s);
}

// the same list pass over the centroid chunks (every query probes every chunk)
void IndexSearch::coarse_list_pass() {
    if (fp8) {
        launch_to_bf16(qvars, nq, d, (int64_t)maxv * qstride, qhi, ix->dpad, s);
        MQVS_HIP(hipGetLastError());
    }
    ListArgs a;
    a.metric = ix->metric;
    a.s = s;
    a.qhi = qhi;
    a.qnorm = qnorms;
    a.nq = nq;
    a.probes = nullptr;  // dense plan: probe r of every query is chunk r
    a.nprobe = (int)ix->cnl;
    a.R = nprobe;
    a.out_rows = probes;
    a.dense = true;
    list_pass(ws.coarse, coarse_layout(ix), a);
}

// mqvs_index_probes: the coarse step's lists, nothing after it
void IndexSearch::probes_only() {
    MQVS_HIP(hipMemcpyAsync(probes_out, probes, sizeof(int64_t) * (size_t)nq * nprobe, hipMemcpyDeviceToHost, s));
    MQVS_HIP(hipMemcpyAsync(ws.host + 6, istat, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    host_wait(s);
    g_istats.pick_overflow = (int32_t)ws.host[6];
}

// ---- the re-rank's bound pruning (the candidates that cannot reach the
// exact top k are not re-ranked; same output): per query, the bound on
// |list-scan value - exact value| for query variant 0.  An fp8 plane takes
// the same bound with the fp8 records of the query (|x8|, |x - x8|, |x|)
// and of the plane: the truncation term |x8| max|ry| + |rx| max|y8| + |rx|
// max|ry| and the accumulation term 2.04 d u |x8| max|y8| (the bf16 MFMA
// sums exact products of the codes' values in fp32, and the scaling by
// 2^-(e_p + e_q) is exact unless the result is subnormal: at most 2^-149
// more, inside the bound's 1e-30 absolute slack).
void IndexSearch::prune_bound() {
    prune = !first_stage && !(flags & MQVS_F_RERANK_ALL) && ix->yrec && k < R;
    if (!prune) return;
    craw = (float *)ws.craw.get(sizeof(float) * (size_t)nq * R);
    ibq = (float *)ws.ibq.get(sizeof(float) * (size_t)nq);
    if (split) qdelta = (float *)ws.qdelta.get(sizeof(float) * (size_t)nq);
    if (fp8) {
        qrec0 = q8rec;
    } else if (!qrec0) {
        qrec0 = (float *)ws.crec.get(sizeof(float) * kMxRec * (size_t)nq);
        launch_to_hi(qvars, nq, d, (int64_t)maxv * qstride, ix->dpad, 1, round_up(nq, 16), nullptr, qrec0, nullptr, s);
    }
    ScanParams bp{};
    bp.nq = nq;
    bp.d = d;
    bp.maxv = 1;
    bp.qnorms = qnorms;
    bp.blas_nq = fnq;
    launch_query_bound(bp, ix->metric, seg->ynorm_max, qrec0, ix->yrec, ibq, nullptr, s);
    MQVS_HIP(hipGetLastError());
}

// The chain starts after the coarse step: beside the coarse batch kernel
// it slowed that kernel by ~20 us, beside the plan and the list scan it
// costs less (mode 3, nprobe 1: 0.564 -> 0.544 ms per batch,
// profiles/r04/index/fork_ab.jsonl).
void IndexSearch::fork_chain() {
    MQVS_HIP(hipEventRecord(ws.fork, s));
    MQVS_HIP(hipStreamWaitEvent(ws.side, ws.fork, 0));
    join_guard.on = true;
    launch_query_prep(dq, nq, d, MQVS_METRIC_COSINE, false, qvars, maxv, qnorms, qmu, qlam, status, ws.side, 2, qdelta);
    MQVS_HIP(hipGetLastError());
    MQVS_HIP(hipEventRecord(ws.join, ws.side));
}

// ---- fine: the probed lists.  A first-stage search takes the pass's ids
// and approximate distances as its result; a two-stage one the candidate
// rows (and, pruning, their scan values) for the re-rank.
void IndexSearch::fine() {
    ListArgs a;
    a.metric = ix->metric;
    a.s = s;
    a.qhi = fp8 ? q8 : qhi;
    a.qnorm = qnorms;
    a.qexp = fp8 ? q8exp : nullptr;
    a.nq = nq;
    a.probes = probes;
    a.nprobe = nprobe;
    a.filter = dfilter;
    a.exists = dexists;
    a.R = R;
    a.ev = tev ? ws.ev : nullptr;
    a.pair_stats = pstats;
    if (first_stage) {
        a.out_rows = out.ids;
        a.id_offset = seg->row_offset;
        a.out_approx = out.dist;
    } else {
        crow = (int64_t *)ws.rows.get(sizeof(int64_t) * (size_t)nq * R);
        a.out_rows = crow;
        a.out_raw = craw;
    }
    fine_stats = list_pass(ws.fine, fine_layout(ix), a);
}

// ---- exact re-rank (needs the whole variant chain)
void IndexSearch::rerank() {
    if (split) {
        MQVS_HIP(hipStreamWaitEvent(s, ws.join, 0));
        join_guard.on = false;
    }
    ScanParams rp{};
    rp.rows = seg->rows;
    rp.row_norms = seg->norms;
    rp.n = seg->n;
    rp.d = d;
    rp.nq = nq;
    rp.blas_nq = fnq;
    rp.qvars = qvars;
    rp.qnorms = qnorms;
    rp.qmu = qmu;
    rp.qlam = qlam;
    rp.maxv = maxv;
    rp.chunk_rows = seg->granule;
    rp.chunk_ord = seg->chunk_ord;
    if (cos && dfilter) {
        // chunk ordinals as mqvs_search computes them under a PREWHERE
        // filter (chunks without a selected row are never searched), so
        // the re-rank picks the same cosine query variant per row
        const int64_t nch = (seg->n + seg->granule - 1) / seg->granule;
        int *o = (int *)ws.ord.get(sizeof(int) * std::max<int64_t>(nch, 1));
        launch_chunk_ordinals(dfilter, seg->nonempty_bits, dexists, seg->n, seg->granule, 1, o, s);
        MQVS_HIP(hipGetLastError());
        rp.chunk_ord = o;
    }
    rp.ord_base = (int)ord_base;
    rp.exists = dexists;
    rp.filter = nullptr;  // the scan applied the filter; candidates pass it
    rp.nonempty = seg->nonempty_bits;
    uint4 *rscr = R > kSortCap ? (uint4 *)ws.fine.large.get(sizeof(uint4) * 2 * (size_t)R * nq) : nullptr;
    RerankPrune pr{};
    pr.count = istat + 1;
    if (prune) {
        pr.raw = craw;
        pr.bq = ibq;
        pr.ymax = seg->ynorm_max;
        pr.qdelta = qdelta;
    }
    launch_rerank_ids(rp, ix->metric, crow, R, k, seg->row_offset, out.ids, out.dist, rscr, s, pr);
    MQVS_HIP(hipGetLastError());
}

// the thread's stats from the pinned words of its last search (after the
// wait that covers them).  A binary search has no plan, pick or re-rank: those
// fields stay 0, and it records nothing between ev[4] and ev[5].
void index_read_stats(IndexWorkspace &ws, mqvs_index_search_stats st, bool tev, bool binary) {
    const int64_t *hs = ws.host;
    st.values = hs[0];
    st.items = hs[1];
    st.plane_bytes = hs[2];
    st.pairs = hs[3];
    if (!binary) {
        st.pick_overflow = (int32_t)hs[6];  // (istat, copied with the status words)
        st.reranked = hs[7];
    }
    float t[5] = {0, 0, 0, 0, 0}, tot = 0;
    if (tev) {
        for (int i = 0; i < (binary ? 4 : 5); ++i) MQVS_HIP(hipEventElapsedTime(&t[i], ws.ev[i], ws.ev[i + 1]));
        MQVS_HIP(hipEventElapsedTime(&tot, ws.ev[0], ws.ev[5]));
    }
    st.coarse_ms = t[0];
    st.plan_ms = binary ? 0 : t[1];
    st.scan_ms = t[2];
    st.select_ms = t[3];
    st.rerank_ms = t[4];
    st.total_ms = tot;
    g_istats = st;
}

// the fine pass's stats and the status words -> the workspace's pinned words
void IndexSearch::queue_stats() {
    int64_t *dstats = fine_stats.words;
    launch_words_to_host(dstats, 4, status, 8, ws.host, reinterpret_cast<int *>(ws.host + 4), s,
                         fine_stats.per_query ? dstats : nullptr, nq);
    MQVS_HIP(hipGetLastError());
}

void IndexSearch::finish_async() {
    const bool variants_matter = !first_stage && ords > maxv;
    launch_async_flags(nullptr, status, variants_matter ? 1 : 0, async_word ? async_word : async_sticky(seg->device, s),
                       s);
    MQVS_HIP(hipGetLastError());
    if (async_word) {
        // the stats land in pinned memory, read after the caller's sync
        // (index_collect_stats)
        queue_stats();
        ws.pending = true;
        ws.pending_tev = tev;
        ws.pending_st = st;
    }
}

int IndexSearch::finish_sync() {
    int *hst = reinterpret_cast<int *>(ws.host + 4);
    if (!dev) {
        // (host outputs: copied before the final wait)
        if (ix->row_ids_map) launch_map_ids(out.ids, (int64_t)nq * k, ix->row_ids_map, s);
        ws.io.finish_begin(out, s);
    }
    queue_stats();
    host_wait(s);
    if (const int want = first_stage ? 0 : check_variant_chain(*hst, ords, maxv)) return want;
    ws.io.finish_end(out);
    ws.pending = false;
    index_read_stats(ws, st, tev, false);
    return 0;
}

// the stats of this thread's last ASYNC search with a flag word of the
// caller's on `device`, once the caller has synchronised its stream
void index_collect_stats(int device) {
    DeviceGuard guard(device);
    IndexWorkspace &ws = index_workspace(device);
    if (!ws.pending) return;
    ws.pending = false;
    index_read_stats(ws, ws.pending_st, ws.pending_tev, false);
}

// nprobe of a search of either kind: the `nprobe` parameter, else from the
// search's alpha (the `alpha` parameter, else the index's)
int search_nprobe(const mqvs_index *ix, const std::map<std::string, std::string> &pm) {
    const double alpha = num_param(pm, "alpha", ix->alpha, 1.0, 4.0);
    return pm.count("nprobe") ? (int)num_param(pm, "nprobe", 1, 1, (double)std::min<int64_t>(ix->nlist, kSortCap))
                              : nprobe_of(ix, alpha);
}

// The driver: resolves the search parameters, splits into query sub-batches
// where one batch's scratch would not fit, admits the search to the workspace
// and runs the stages; a cosine chain that outgrew its variant table runs
// them again with the larger one.
// formula_nq: the call's batch size, which selects the exact re-rank's
// distance formula (0: nq; query sub-batches keep the call's, see search.hip)
// ord_base: the cosine chunk-ordinal base of a row-range shard (< 0:
// row_offset / granule); the sub-batches and the re-run keep it.  async_word:
// an ASYNC search's outcome flags go there instead of the sticky word.
// probes_out (mqvs_index_probes): the search ends after the coarse step, whose
// probes[nq][nprobe] are copied there.
void search_index_impl(mqvs_index *ix, const float *queries, int nq, int k, const char *params, const uint8_t *filter,
                       const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags,
                       hipStream_t user_stream, int formula_nq, int maxv_hint, int64_t ord_base, int *async_word,
                       int64_t *probes_out) {
    const int fnq = formula_nq > 0 ? formula_nq : nq;
    check_search_args(ix, "index", ix && ix->binary ? "binary index: search it with mqvs_index_search_binary" : nullptr,
                      nq, k, queries, out_ids, out_dist);
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "nprobe", "num_reorder"}, "search");
    const bool first_stage = flags & MQVS_F_FIRST_STAGE;
    const int nprobe = search_nprobe(ix, pm);
    // num_reorder up to kSortCap sorts in LDS; above it (k > 2048 by default,
    // up to kLargeCap) through global scratch
    const int R = first_stage ? k
                              : (int)num_param(pm, "num_reorder",
                                               (double)std::min(k > kSortCap / 2 ? kLargeCap : kSortCap, std::max(2 * k, 64)),
                                               (double)std::max(k, 1), (double)kLargeCap);
    mqvs_index_search_stats st{};
    st.nq = nq;
    st.k = k;
    st.nprobe = nprobe;
    st.num_reorder = R;
    g_istats = st;
    if (nq == 0 || k == 0) return;
    if (R > kSortCap) {
        // the select and the re-rank each take 2 R records of scratch per
        // query: query sub-batches of <= 1 GB of it
        const int qb = (int)std::max<int64_t>(1, (int64_t)scratch_budget() / 16 / (2 * (int64_t)R));
        if (nq > qb) {
            const int d = ix->seg->d;
            for_query_batches(nq, qb, [&](int q0, int m) {
                search_index_impl(ix, queries + (size_t)q0 * d, m, k, params, filter, exists,
                                  out_ids + (size_t)q0 * k, out_dist + (size_t)q0 * k, flags, user_stream, fnq, 0,
                                  ord_base, async_word, probes_out ? probes_out + (size_t)q0 * nprobe : nullptr);
            });
            // (the counters and times left are the last sub-batch's: the
            // binary driver sums its sub-batches', this one never has)
            g_istats.nq = nq;
            return;
        }
    }

    SearchAdmission adm(ix->seg, user_stream);
    // (declared after the admission: its join guard runs before the scope is released)
    IndexSearch search(ix, adm.ws, adm.s, queries, nq, k, filter, exists, out_ids, out_dist, flags, fnq, nprobe, R,
                       maxv_hint, ord_base, async_word, probes_out, st);
    if (const int want = search.run())
        search_index_impl(ix, queries, nq, k, params, filter, exists, out_ids, out_dist, flags, user_stream, fnq, want,
                          ord_base, async_word, probes_out);
}

}  // namespace mqvs
