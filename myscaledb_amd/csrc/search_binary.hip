// search_binary.hip -- the FLAT search of a binary (FixedString) segment:
// vectorScanWithoutIndex<BinaryVector> for one part
// (MergeTreeVSManager.cpp:1188-1273 filtered gather, :1395-1425 whole chunks)
// on the same probe / threshold / append / select pipeline as the float VALU
// path, with the popcount scan of kernels_binary.hip and the L2 ordering key
// (both binary distances are ascending and finite).  No granule chunking is
// needed: the reference's per-chunk strict merges keep the k best by
// (distance, row) over the part, like the float L2 path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>

#include "workspace.h"

namespace mqvs {

// mqvs_set_binary_batch: calls of nq >= this take the i8 MFMA scan
// (kernels_binary_mfma.hip) instead of the popcount scan; 0 = never
static std::atomic<int32_t> g_binary_batch{0};

void search_binary(mqvs_segment *seg, const uint8_t *queries, int nq, int k, int metric, const uint8_t *filter,
                   const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags,
                   hipStream_t user_stream) {
    check_search_args(seg, "segment", seg && !seg->binary ? "Float32 segment: search it with mqvs_search" : nullptr,
                      nq, k, queries, out_ids, out_dist);
    if (metric != MQVS_METRIC_HAMMING && metric != MQVS_METRIC_JACCARD)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Binary Vector");
    mqvs_search_stats st{};
    search_stats() = st;
    if (nq == 0 || k == 0) return;
    if (k > kSortCap) {
        const int qb = large_k_batch(seg->n, k);
        if (nq > qb) {
            for_query_batches(nq, qb, [&](int q0, int m) {
                search_binary(seg, queries + (size_t)q0 * seg->code_bytes, m, k, metric, filter, exists,
                              out_ids + (size_t)q0 * k, out_dist + (size_t)q0 * k, flags, user_stream);
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
    const int64_t n = seg->n;
    const bool timing = timing_on(flags);
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[0], s));

    uint32_t *qc = (uint32_t *)ws.io.queries.get((size_t)nq * seg->code_words * 4);
    upload_codes(qc, seg->code_words, queries, seg->code_bytes, nq, dev, s);
    const CallIO::In in = ws.io.in(nullptr, 0, filter, exists, (n + 7) / 8, dev, s);
    const uint8_t *dfilter = in.filter, *dexists = in.exists;
    const CallIO::Out out = ws.io.out((size_t)nq * k, dev, out_ids, out_dist);
    int64_t *dids = out.ids;
    float *ddist = out.dist;

    // candidate capacity and probe size as the float path (search.hip)
    constexpr int64_t tile_rows = kSmallRows;
    const int cap = cand_capacity(nq, k);
    const int64_t target_cands = std::min<int64_t>(cap / 3, std::max<int64_t>(16384, 2 * (int64_t)k));
    uint4 *large = k > kSortCap ? (uint4 *)ws.large.get(sizeof(uint4) * 2 * kLargeCap * (size_t)nq) : nullptr;
    int64_t P = n;
    if (n > 32768) {
        P = (int64_t)(((double)k * (double)n) / target_cands) + 1;
        // the refines between main segments keep appends near 2k per segment
        // whatever the probe, so the probe stays short on big parts (its select
        // is one workgroup per query)
        P = std::min<int64_t>(P, std::max<int64_t>(nq <= 8 ? 16384 : 65536, 8 * (int64_t)k));
        P = std::max<int64_t>(P, 8 * (int64_t)k);
        P = round_up(P, tile_rows);
        if (P > n) P = n;
    }
    ScanParams p{};
    p.n = n;
    p.nq = nq;
    p.chunk_rows = seg->granule;
    p.filter = dfilter;
    p.exists = dexists;
    p.codes = seg->codes;
    p.qcodes = qc;
    p.code_words = seg->code_words;
    p.nbits = seg->d;
    uint32_t *tau = (uint32_t *)ws.tau.get(sizeof(uint32_t) * nq);
    int *count = (int *)ws.count.get(sizeof(int) * nq);
    Cand *cand = (Cand *)ws.cand.get(sizeof(Cand) * (size_t)nq * cap);
    int *overflow = (int *)ws.overflow.get(sizeof(int) * 4);
    p.tau = tau;
    p.cand_count = count;
    p.cand = cand;
    p.cand_cap = cap;
    p.probe = (float *)ws.probe.get(sizeof(float) * (size_t)nq * std::max<int64_t>(P, 1));
    p.probe_ld = P;
    // the scan kernel of this call: the popcount scan, or (opt-in) the i8 MFMA
    // scan over the queries expanded to 0/1 bytes -- the same values and
    // candidates, so everything around the scan is shared
    const int32_t batch_min = g_binary_batch.load(std::memory_order_relaxed);
    const bool mfma = batch_min > 0 && nq >= batch_min;
    BinPlane qexp{};
    if (mfma) {
        uint8_t *qplane = (uint8_t *)ws.bin_qplane.get(bin_plane_bytes(nq, seg->code_words));
        uint32_t *qpop = (uint32_t *)ws.bin_qpop.get(sizeof(uint32_t) * (size_t)round_up(nq, 16));
        launch_bin_expand(qc, nq, seg->code_words, qplane, qpop, s);
        MQVS_HIP(hipGetLastError());
        qexp.plane = qplane;
        qexp.pop = qpop;
    }
    auto scan = [&](int64_t b, int64_t e, bool probe, bool strict) {
        if (e <= b) return;
        p.row_begin = b;
        p.row_end = e;
        p.tiles = (e - b + tile_rows - 1) / tile_rows;
        p.tiles_per_chunk = 0;
        p.tile_rows = tile_rows;
        p.tau_strict = strict ? 1 : 0;
        if (mfma)
            launch_scan_binary_mfma(p, qexp, metric, probe, s);
        else
            launch_scan_binary(p, metric, probe, s);
        MQVS_HIP(hipGetLastError());
    };
    constexpr int kOrder = MQVS_METRIC_L2;  // ascending finite values: ord_asc key, (key, row) ties
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[5], s));
    scan(0, P, true, false);
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[1], s));
    launch_fill2((uint32_t *)count, nq, 0u, nullptr, 0, 0u, s);
    launch_probe_select(p.probe, P, P, nq, k, kOrder, tau, count, cand, cap, 0, nullptr, s);
    MQVS_HIP(hipGetLastError());
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[2], s));
    Cand *alt = (Cand *)ws.cand2.get(sizeof(Cand) * (size_t)nq * cap);
    int *calt = (int *)ws.count2.get(sizeof(int) * nq);
    {
        // segments grow x4: each refine costs a launch, and appends per
        // segment stay near (growth x k) with the threshold refined
        int64_t b = P, seg_rows = std::max<int64_t>(2 * P, tile_rows);
        int segs = 0;
        while (b < n) {
            const int64_t e = std::min(n, round_up(b + seg_rows, tile_rows));
            scan(b, e, false, true);
            b = e;
            seg_rows *= 4;
            ++segs;
            if (b < n) {
                launch_refine(cand, count, cap, nq, k, kOrder, false, nullptr, tau, nullptr, alt, calt, s);
                MQVS_HIP(hipGetLastError());
                std::swap(cand, alt);
                std::swap(count, calt);
                p.cand = cand;
                p.cand_count = count;
            }
        }
        st.segments = segs;
    }
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[3], s));
    launch_fill2((uint32_t *)overflow, 4, 0u, nullptr, 0, 0u, s);
    launch_final_select(cand, count, cap, nq, k, kOrder, 0, seg->row_offset, dids, ddist, overflow, large, s);
    MQVS_HIP(hipGetLastError());
    if (timing) MQVS_HIP(hipEventRecord(ws.ev[4], s));
    st.path = mfma ? 4 : 3;  // binary scan: i8 MFMA / popcount
    st.probe_rows = P;
    st.main_rows = n - P;
    st.rows_scanned = n;
    st.nq = nq;
    st.k = k;
    const bool async = dev && (flags & MQVS_F_ASYNC);
    if (async) {
        launch_async_flags(overflow, nullptr, 0, sticky_word(ws, s), s);
        MQVS_HIP(hipGetLastError());
    } else {
        ws.io.finish_begin(out, s);
        MQVS_HIP(hipMemcpyAsync(ws.host_flags, overflow, sizeof(int), hipMemcpyDeviceToHost, s));
        host_wait(s);
        OverflowRescan r{cand, alt,   count, calt, cap, nq, k, kOrder, tau, overflow, 0, seg->row_offset,
                         dids, ddist, large, n,    tile_rows};
        st.rescans = rescan_on_overflow(ws, r, s, [&](int64_t b, int64_t e, Cand *to, int *to_count) {
            p.cand = to;
            p.cand_count = to_count;
            scan(b, e, false, false);
        });
        if (st.rescans)
            ws.io.finish(out, s);
        else
            ws.io.finish_end(out);
        if (timing) read_search_times(ws, st, 0);  // (no per-segment events here)
    }
    search_stats() = st;
}

}  // namespace mqvs

extern "C" {

int mqvs_set_binary_batch(int32_t min_nq) {
    if (min_nq < 0) return MQVS_ERR_BAD_ARGUMENTS;
    mqvs::g_binary_batch.store(min_nq, std::memory_order_relaxed);
    return MQVS_OK;
}

int mqvs_binary_batch(int32_t *min_nq) {
    if (min_nq) *min_nq = mqvs::g_binary_batch.load(std::memory_order_relaxed);
    return MQVS_OK;
}

}  // extern "C"

