// index_search_binary.hip -- the binary index search of libmqvs
// (mqvs_index_search_binary, mqvs_index_probes_binary; the build:
// index_build.hip, the C glue: index.hip).
//
// Search: the nprobe nearest centroids by (Hamming, list id) (every list, with
// no ranking, when nprobe == nlist), the probed lists scanned with the search
// metric, filter ∩ row_exists and the b < nBit rule applied per position, and
// the k best by (distance, part row) taken by the brute-force path's final
// select (which keeps the smallest rows of a tie group at the k-th key however
// large the group is).  Binary distances are exact, so there is no
// approximate stage and nothing is re-ranked.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "index_internal.h"

namespace mqvs {

// ---- the search of one query batch --------------------------------------------
// Stages over the search's state, as IndexSearch (index_search.hip): run()
// queues them in order on one stream.  The parameters are resolved, and the
// workspace admitted, by search_binary_index_impl below.
struct BinaryIndexSearch {
    // ---- call inputs
    mqvs_index *const ix;
    mqvs_segment *const seg;
    IndexWorkspace &ws;
    const hipStream_t s;
    const uint8_t *const queries;
    const int nq, k;
    const uint8_t *const filter, *const exists;
    int64_t *const out_ids;
    float *const out_dist;
    const uint32_t flags;
    const int metric, nprobe;  // as resolved from the search parameters
    const int64_t cap;         // a query's record region
    // mqvs_index_probes_binary: the coarse step's probes[nq][nprobe] are
    // copied there and the search ends
    int64_t *const probes_out;
    // ---- derived constants
    const bool dev, async, tev;
    const bool rank;  // fewer probes than lists: the centroids are ranked
    const int cw;
    // ---- device pointers
    uint32_t *qc = nullptr;  // the queries, zero-padded [nq][code_words]
    const uint8_t *dfilter = nullptr, *dexists = nullptr;
    CallIO::Out out{};
    // [0] the final select's overflow word (never set: a region holds every
    // position of its lists)
    int *status = nullptr;
    int *count = nullptr;
    int64_t *probes = nullptr;
    Cand *cand = nullptr;
    int64_t *dstats = nullptr;
    // ---- stats
    mqvs_index_search_stats st;

    BinaryIndexSearch(mqvs_index *index, IndexWorkspace &w, hipStream_t stream, const uint8_t *q, int nq_, int k_,
                      const uint8_t *filter_, const uint8_t *exists_, int64_t *ids, float *dist, uint32_t flags_,
                      int metric_, int nprobe_, int64_t cap_, int64_t *probes_out_,
                      const mqvs_index_search_stats &header)
        : ix(index), seg(index->seg), ws(w), s(stream), queries(q), nq(nq_), k(k_), filter(filter_), exists(exists_),
          out_ids(ids), out_dist(dist), flags(flags_), metric(metric_), nprobe(nprobe_), cap(cap_),
          probes_out(probes_out_), dev(flags_ & MQVS_F_DEVICE_PTRS), async(dev && (flags_ & MQVS_F_ASYNC)),
          tev(timing_on(flags_)), rank(nprobe_ < index->nlist), cw(index->seg->code_words), st(header) {}

    void stage_inputs();
    void coarse();
    void probes_only();
    void scan();
    void select();
    void finish();

    void run() {
        stage_inputs();
        coarse();
        if (probes_out) {
            probes_only();
            return;
        }
        scan();
        select();
        MQVS_HIP(hipEventRecord(ws.ev[5], s));
        finish();
    }
};

void BinaryIndexSearch::stage_inputs() {
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[0], s));
    qc = (uint32_t *)ws.io.queries.get(sizeof(uint32_t) * (size_t)nq * cw);
    upload_codes(qc, cw, queries, seg->code_bytes, nq, dev, s);
    const CallIO::In in = ws.io.in(nullptr, 0, filter, exists, (seg->n + 7) / 8, dev, s);
    dfilter = in.filter;
    dexists = in.exists;
    out = ws.io.out((size_t)nq * k, dev, out_ids, out_dist);
    status = (int *)ws.status.get(sizeof(int) * 8);
    count = (int *)ws.fine.lcount.get(sizeof(int) * nq);
    launch_fill2(reinterpret_cast<uint32_t *>(status), 8, 0u, reinterpret_cast<uint32_t *>(count), nq, 0u, s);
}

void BinaryIndexSearch::coarse() {
    probes = (int64_t *)ws.probes.get(sizeof(int64_t) * (size_t)nq * nprobe);
    if (rank) {
        auto *cd = (uint32_t *)ws.pdist.get(sizeof(uint32_t) * (size_t)nq * ix->nlist);
        launch_bivf_coarse(ix->bcent, (int)ix->nlist, cw, qc, nq, nprobe, cd, probes, s);
    } else {
        launch_iota_probes(probes, nq, nprobe, s);
    }
    MQVS_HIP(hipGetLastError());
    if (tev) {
        MQVS_HIP(hipEventRecord(ws.ev[1], s));
        MQVS_HIP(hipEventRecord(ws.ev[2], s));
    }
}

void BinaryIndexSearch::probes_only() {
    MQVS_HIP(hipMemcpyAsync(probes_out, probes, sizeof(int64_t) * (size_t)nq * nprobe, hipMemcpyDeviceToHost, s));
    MQVS_HIP(hipEventRecord(ws.ev[5], s));
    host_wait(s);
}

// ---- the probed lists
void BinaryIndexSearch::scan() {
    BivfParams p{};
    p.plane = ix->bplane;
    p.perm = ix->perm;
    p.list_off = ix->list_off;
    p.nlist = (int)ix->nlist;
    p.code_words = cw;
    p.nbits = seg->d;
    p.nq = nq;
    p.nprobe = nprobe;
    p.nch = (int)((ix->max_list + 255) / 256);
    p.probes = probes;
    p.qcodes = qc;
    p.filter = dfilter;
    p.exists = dexists;
    p.cand = cand = (Cand *)ws.fine.cand.get(sizeof(Cand) * (size_t)nq * cap);
    p.cand_count = count;
    p.cand_cap = (int)cap;
    dstats = (int64_t *)ws.fine.stats.get(sizeof(int64_t) * 4);
    launch_bivf_scan(p, metric, dstats, s);
    MQVS_HIP(hipGetLastError());
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[3], s));
}

void BinaryIndexSearch::select() {
    uint4 *large = k > kSortCap ? (uint4 *)ws.fine.large.get(sizeof(uint4) * 2 * kLargeCap * (size_t)nq) : nullptr;
    // ascending finite values: the L2 ordering key, (key, row) ties
    launch_final_select(cand, count, (int)cap, nq, k, MQVS_METRIC_L2, 0, seg->row_offset, out.ids, out.dist, status,
                        large, s);
    MQVS_HIP(hipGetLastError());
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[4], s));
}

void BinaryIndexSearch::finish() {
    // decoupled part: results in the new part's row ids
    if (ix->row_ids_map) launch_map_ids(out.ids, (int64_t)nq * k, ix->row_ids_map, s);
    if (async) {
        launch_async_flags(status, nullptr, 0, async_sticky(seg->device, s), s);
        MQVS_HIP(hipGetLastError());
        return;
    }
    int *hst = reinterpret_cast<int *>(ws.host + 4);
    ws.io.finish_begin(out, s);
    launch_words_to_host(dstats, 4, status, 8, ws.host, hst, s);
    MQVS_HIP(hipGetLastError());
    host_wait(s);
    if (*hst) fail(MQVS_ERR_DEVICE, "binary index search: a query's record region overflowed");
    ws.io.finish_end(out);
    index_read_stats(ws, st, tev, /*binary=*/true);
}

// The driver: checks, search parameters, query sub-batches under the scratch
// budget, admission to the workspace, then the stages.
void search_binary_index_impl(mqvs_index *ix, const uint8_t *queries, int nq, int k, const char *params,
                              const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                              uint32_t flags, hipStream_t user_stream, int64_t *probes_out) {
    check_search_args(ix, "index", ix && !ix->binary ? "Float32 index: search it with mqvs_index_search" : nullptr, nq,
                      k, queries, out_ids, out_dist);
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "nprobe", "num_reorder", "metric"}, "search");
    const int metric = pm.count("metric") ? binary_metric_of(pm.at("metric"), "metric") : ix->metric;
    const int nprobe = search_nprobe(ix, pm);
    // (accepted and ignored: the scan is exact, nothing is re-ordered)
    (void)num_param(pm, "num_reorder", 1, 1, (double)kLargeCap);
    search_binary_index_impl(ix, queries, nq, k, metric, nprobe, filter, exists, out_ids, out_dist, flags, user_stream,
                             probes_out);
}

// The same with the search parameters resolved (the driver above; an index
// group's per-part route): metric Hamming or Jaccard, 1 <= nprobe <= nlist.
void search_binary_index_impl(mqvs_index *ix, const uint8_t *queries, int nq, int k, int metric, int nprobe,
                              const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                              uint32_t flags, hipStream_t user_stream, int64_t *probes_out) {
    mqvs_index_search_stats st{};
    st.nq = nq;
    st.k = k;
    st.nprobe = nprobe;
    g_istats = st;
    if (nq == 0 || k == 0) return;

    mqvs_segment *seg = ix->seg;
    // a query's records: at most every position of its probed lists
    const int64_t cap = binary_index_cap(ix, nprobe);
    // query sub-batches under the scratch budget (records, centroid
    // distances, the large-k sort scratch); the stats are the sub-batches' sums
    const int64_t perq = binary_index_scratch(ix, nprobe) + (k > kSortCap ? (int64_t)sizeof(uint4) * 2 * kLargeCap : 0);
    const int qb = (int)std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)scratch_budget() / perq));
    if (nq > qb) {
        mqvs_index_search_stats sum = st;
        for_query_batches(nq, qb, [&](int q0, int m) {
            search_binary_index_impl(ix, queries + (size_t)q0 * seg->code_bytes, m, k, metric, nprobe, filter, exists,
                                     out_ids + (size_t)q0 * k, out_dist + (size_t)q0 * k, flags, user_stream,
                                     probes_out ? probes_out + (size_t)q0 * nprobe : nullptr);
            sum.coarse_ms += g_istats.coarse_ms;
            sum.scan_ms += g_istats.scan_ms;
            sum.select_ms += g_istats.select_ms;
            sum.total_ms += g_istats.total_ms;
            sum.values += g_istats.values;
            sum.items += g_istats.items;
            sum.plane_bytes += g_istats.plane_bytes;
            sum.pairs += g_istats.pairs;
        });
        g_istats = sum;
        return;
    }

    SearchAdmission adm(seg, user_stream);
    BinaryIndexSearch search(ix, adm.ws, adm.s, queries, nq, k, filter, exists, out_ids, out_dist, flags, metric, nprobe,
                             cap, probes_out, st);
    search.run();
}

}  // namespace mqvs
