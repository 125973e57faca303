// index_build.hip -- the index builds of libmqvs (mqvs_index_build; the search:
// index_search.hip and index_search_binary.hip, save / load: index_blob.hip,
// the C glue: index.hip).
//
// Float build (all on the GPU except the sample's counting sort per k-means
// step):
//   k-means over a row sample: assignment = FLAT top-1 search of the sample
//   rows against a centroid segment (the MFMA pre-filter path of mqvs_search),
//   deterministic ordered means (k_centroid_mean); cosine centroids are
//   re-normalised (spherical k-means).  Every row is then assigned to its
//   nearest centroid; finish_index groups the rows by list on the device (row
//   order within a list) and writes the lists back to back as a bf16 plane.
// Binary build: k-majority lists over the codes, below.
// Both resolve the same build parameters (BuildShape) and run in the same
// timed frame that owns the index until it is finished (timed_build); the
// list count's auto-tuning (build_auto) wraps the float build.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "index_internal.h"

namespace mqvs {

// nearest centroid of `m` rows (device, row-major d) -> assign[m] (int64, -1 = none)
static void assign_rows(mqvs_index *ix, mqvs_segment *cseg, const float *rows, int64_t m, int64_t *assign,
                        float *scratch_dist, hipStream_t s) {
    constexpr int64_t kBatch = 8192;
    for (int64_t b = 0; b < m; b += kBatch) {
        const int nb = (int)std::min(kBatch, m - b);
        search_internal(cseg, rows + b * ix->seg->d, nb, 1, ix->coarse_metric, nullptr, nullptr, assign + b,
                        scratch_dist, MQVS_F_DEVICE_PTRS, s);
    }
}

// stable counting sort of assign[m] (list ids, -1 dropped): order (indices
// into the assigned set, ascending within a list) and offsets [L+1] (the
// k-means steps over the sample; the rows themselves: finish_index)
static void group_by_list(const std::vector<int64_t> &assign, int64_t L, int64_t pad, std::vector<int32_t> &order,
                          std::vector<int64_t> &off) {
    std::vector<int64_t> cnt(L + 1, 0);
    for (size_t i = 0; i < assign.size(); ++i) {
        const int64_t a = assign[i];
        if (a >= 0 && a < L) ++cnt[a];
    }
    off.assign(L + 1, 0);
    for (int64_t l = 0; l < L; ++l) off[l + 1] = off[l] + round_up(cnt[l], pad);
    order.assign(off[L], -1);
    std::vector<int64_t> cur(off.begin(), off.end() - 1);
    for (size_t i = 0; i < assign.size(); ++i) {
        const int64_t a = assign[i];
        if (a >= 0 && a < L) order[cur[a]++] = (int32_t)i;
    }
}

static mqvs_index *build_auto(mqvs_segment *seg, const char *index_type, const char *params);
constexpr int64_t kAutoNlistMinRows = 1 << 20;  // smaller parts take the default list count

static mqvs_index *build_binary_impl(mqvs_segment *seg, const char *params);

// the list scan keeps a tile of at least 16 bf16 queries in LDS
// (ivf_scan_lds): rows too wide for that cannot be searched
void check_index_width(mqvs_segment *seg) {
    const int d = seg->d;
    DeviceGuard guard(seg->device);
    const int64_t lim = device_lds_bytes();
    if (ivf_fit_qg(16, round_up(d, kBfK), lim) == 0) {
        int64_t dmax = (lim / 16 - 32) / 2 / kBfK * kBfK;
        fail(MQVS_ERR_BAD_ARGUMENTS, "dimension " + std::to_string(d) + " is too wide for an index: the list scan's " +
                                         "16-query tile must fit the workgroup's " + std::to_string(lim) +
                                         " bytes of LDS (at most " + std::to_string(dmax) + " dimensions)");
    }
}

// ---- the tail of every build and of mqvs_index_load ---------------------------
// From the centroids (ix->cent for a float index, ix->bcent for a binary one)
// and the canonical assignment -- assign[n] on the device: each row's list, -1
// for a row in no list -- to the finished index: the rows grouped by list on
// the device (kernels_ivf_build.hip: k_grp_*), then everything derived from that:
// the list plane (bf16, or fp8 codes + scale exponents) and |y|^2 in list
// order, the plane's norm maxima and the coarse quantizer's centroid lists
// (float), or the codes in list order (binary).  ix: seg, binary, metric,
// nlist, dpad, plane_fmt set.  The assignment is
// range-checked by the kernel that first reads it, and the verdict is read
// before anything is sized by or indexed with it: from a blob (from_blob) a
// bad value is the blob's fault, from a build the device's.
void finish_index(mqvs_index *ix, const int32_t *assign, bool from_blob, hipStream_t s) {
    mqvs_segment *seg = ix->seg;
    const int64_t n = seg->n, L = ix->nlist;
    const int d = seg->d;
    const uint8_t *nonempty = ix->binary ? nullptr : seg->nonempty_bits;
    TmpBuf cnt(sizeof(int) * L), fill(sizeof(int) * L), info(sizeof(int64_t) * 8);
    MQVS_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int) * L, s));
    MQVS_HIP(hipMemsetAsync(fill.p, 0, sizeof(int) * L, s));
    MQVS_HIP(hipMemsetAsync(info.p, 0, sizeof(int64_t) * 8, s));
    int *status = (int *)(info.as<int64_t>() + 6);
    ix->list_off = dalloc<int64_t>(ix, L + 1);
    launch_grp_count(assign, n, L, nonempty, !ix->binary, cnt.as<int>(), status, s);
    launch_grp_scan(cnt.as<int>(), L, ix->binary ? 1 : kIvfPad, ix->list_off, info.as<int64_t>(), status, s);
    MQVS_HIP(hipGetLastError());
    int64_t h[5] = {};
    MQVS_HIP(hipMemcpyAsync(h, info.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MQVS_HIP(hipStreamSynchronize(s));
    if (h[4]) {
        const char *what = (h[4] & kGrpStatusBadRange) ? "a list id outside [-1, nlist)" : "a row of a binary index in no list";
        fail(from_blob ? MQVS_ERR_ILLEGAL_COLUMN : MQVS_ERR_DEVICE,
             std::string(from_blob ? "index blob: the assignment holds " : "index build: the assignment holds ") + what);
    }
    ix->npos = h[0];
    ix->max_list = h[1];
    ix->rows_indexed = h[2];
    ix->perm = dalloc<int32_t>(ix, ix->npos);
    {
        const int64_t max_rows = h[3];
        TmpBuf tmp(max_rows > kSortCap ? sizeof(int32_t) * (size_t)ix->npos : 0);
        if (ix->npos > 0) MQVS_HIP(hipMemsetAsync(ix->perm, 0xFF, sizeof(int32_t) * (size_t)ix->npos, s));
        launch_grp_scatter(assign, n, L, nonempty, ix->list_off, fill.as<int>(), ix->perm, s);
        const int32_t *sorted = launch_grp_sort(ix->perm, tmp.as<int32_t>(), ix->list_off, cnt.as<int>(), L, ix->npos,
                                                max_rows, s);
        MQVS_HIP(hipGetLastError());
        if (sorted != ix->perm)
            MQVS_HIP(hipMemcpyAsync(ix->perm, sorted, sizeof(int32_t) * (size_t)ix->npos, hipMemcpyDeviceToDevice, s));
        MQVS_HIP(hipStreamSynchronize(s));  // (tmp)
    }
    if (ix->binary) {
        ix->bplane = dalloc<uint32_t>(ix, (size_t)ix->npos * seg->code_words);
        launch_bivf_gather(seg->codes, seg->code_words, ix->perm, ix->npos, ix->bplane, s);
        MQVS_HIP(hipGetLastError());
        return;
    }
    ix->pnorm = dalloc<float>(ix, ix->npos);
    ix->yrec = dalloc<float>(ix, kMxRec);
    MQVS_HIP(hipMemsetAsync(ix->yrec, 0, sizeof(float) * kMxRec, s));
    if (ix->plane_fmt == MQVS_INDEX_PLANE_FP8) {
        // codes, scale exponents, |y|^2 and the norm maxima of the indexed
        // positions in one pass (a non-finite row makes them infinite)
        ix->plane8 = dalloc<uint8_t>(ix, (size_t)ix->npos * ix->dpad);
        ix->pscale = dalloc<int16_t>(ix, ix->npos);
        launch_to_fp8(seg->rows, d, d, ix->perm, ix->npos, ix->dpad, ix->plane8, nullptr, ix->pscale, seg->norms,
                      ix->pnorm, nullptr, ix->yrec, s);
        MQVS_HIP(hipGetLastError());
    } else {
        ix->plane = dalloc<uint16_t>(ix, (size_t)ix->npos * ix->dpad);
        launch_ivf_pack(seg->rows, seg->norms, d, ix->perm, ix->npos, ix->dpad, ix->plane, ix->pnorm, s);
        MQVS_HIP(hipGetLastError());
        // the plane's norm maxima (the same bf16 rounding as k_ivf_pack; empty
        // arrays' FLT_MAX rows make them infinite, which turns the re-rank's
        // bound pruning off)
        launch_to_hi(seg->rows, n, d, d, ix->dpad, 1, round_up(n, 16), nullptr, nullptr, ix->yrec, s);
        MQVS_HIP(hipGetLastError());
    }
    // ---- coarse quantizer as lists of kCoarseChunk centroids
    ix->cnl = (L + kCoarseChunk - 1) / kCoarseChunk;
    std::vector<int64_t> coff(ix->cnl + 1, 0);
    std::vector<int32_t> cperm;
    for (int64_t j = 0; j < ix->cnl; ++j) {
        const int64_t b = j * kCoarseChunk, e = std::min(L, b + kCoarseChunk);
        for (int64_t c = b; c < e; ++c) cperm.push_back((int32_t)c);
        while ((int64_t)cperm.size() % kIvfPad) cperm.push_back(-1);
        coff[j + 1] = (int64_t)cperm.size();
        ix->cmax = std::max(ix->cmax, coff[j + 1] - coff[j]);
    }
    ix->cnpos = (int64_t)cperm.size();
    ix->cperm = dalloc<int32_t>(ix, ix->cnpos);
    ix->clist_off = dalloc<int64_t>(ix, ix->cnl + 1);
    ix->cplane = dalloc<uint16_t>(ix, (size_t)ix->cnpos * ix->dpad);
    ix->cpnorm = dalloc<float>(ix, ix->cnpos);
    MQVS_HIP(hipMemcpyAsync(ix->cperm, cperm.data(), sizeof(int32_t) * ix->cnpos, hipMemcpyHostToDevice, s));
    MQVS_HIP(hipMemcpyAsync(ix->clist_off, coff.data(), sizeof(int64_t) * (ix->cnl + 1), hipMemcpyHostToDevice, s));
    launch_ivf_pack(ix->cent->rows, ix->cent->norms, d, ix->cperm, ix->cnpos, ix->dpad, ix->cplane, ix->cpnorm, s);
    MQVS_HIP(hipGetLastError());
    MQVS_HIP(hipStreamSynchronize(s));  // cperm / coff are host temporaries
}

// ---- what the two builds share ---------------------------------------------------

// The build parameters both kinds resolve the same way from (params, rows).
struct BuildShape {
    int64_t L;    // nlist
    int64_t S;    // rows of the training sample
    int iters;    // kmeans_iters
    float alpha;  // the index's default search alpha
};

static BuildShape build_shape(const std::map<std::string, std::string> &pm, int64_t n) {
    BuildShape b{};
    // lists of about 256 rows (at most 65536 lists): fine enough that data of
    // many small clusters (generator mode 3: 65536 centres of ~150 rows)
    // keeps its neighbours in one or two lists; n / 1000 left mode 3 needing
    // 512 of 10000 lists for recall 0.95 (profiles/r03/index)
    const int64_t dflt_nlist = std::max<int64_t>(1, std::min<int64_t>(65536, (n + 128) / 256));
    b.L = (int64_t)num_param(pm, "nlist", (double)dflt_nlist, 1, 1 << 20);
    if (n > 0 && b.L > n) fail(MQVS_ERR_BAD_ARGUMENTS, "nlist must not exceed the number of rows");
    b.iters = (int)num_param(pm, "kmeans_iters", 8, 0, 1000);
    // training sample: 64 rows per list up to 1M rows, at least 16 per list
    // (65536 lists: 1M rows, build 9.7 -> 4.1 s at equal recall, profiles/r03/index)
    const int64_t dflt_sample =
        std::min<int64_t>(n, std::max<int64_t>(16 * b.L, std::min<int64_t>(64 * b.L, 1 << 20)));
    b.S = std::max<int64_t>(std::min<int64_t>(n, (int64_t)num_param(pm, "sample", (double)dflt_sample, 1, 1e12)),
                            std::min<int64_t>(n, b.L));
    b.alpha = (float)num_param(pm, "alpha", 3.0, 1.0, 4.0);
    return b;
}

// a timing event that lives as long as its scope
struct TimingEvent {
    hipEvent_t e = nullptr;
    TimingEvent() { MQVS_HIP(hipEventCreate(&e)); }
    ~TimingEvent() { (void)hipEventDestroy(e); }
    TimingEvent(const TimingEvent &) = delete;
    TimingEvent &operator=(const TimingEvent &) = delete;
};

// The frame of a build: on the segment's device and the thread's stream,
// body(ix, s) fills a new index of `seg`, which the frame owns until the body
// has returned and its work has drained (a throw frees it); build_ms is the
// stream time in between.
template <typename Body>
static mqvs_index *timed_build(mqvs_segment *seg, Body &&body) {
    DeviceGuard guard(seg->device);
    hipStream_t s = thread_stream(seg->device);
    TimingEvent e0, e1;
    MQVS_HIP(hipEventRecord(e0.e, s));
    std::unique_ptr<mqvs_index, void (*)(mqvs_index *)> ix(new mqvs_index(), free_index);
    ix->seg = seg;
    body(ix.get(), s);
    MQVS_HIP(hipEventRecord(e1.e, s));
    MQVS_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    MQVS_HIP(hipEventElapsedTime(&ms, e0.e, e1.e));
    ix->build_ms = ms;
    return ix.release();
}

mqvs_index *build_impl(mqvs_segment *seg, const char *index_type, const char *params) {
    if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
    std::string type = index_type ? index_type : (seg->binary ? "BINARYMSTG" : "MSTG");
    for (auto &ch : type) ch = (char)std::toupper((unsigned char)ch);
    const bool btype = type == "BINARYMSTG" || type == "BINARYIVF";
    if (!btype && type != "MSTG" && type != "IVFFLAT")
        fail(MQVS_ERR_NOT_IMPLEMENTED,
             "index type `" + type + "` is not implemented (MSTG, IVFFLAT, BINARYMSTG, BINARYIVF)");
    if (btype != seg->binary)
        fail(MQVS_ERR_LOGICAL, "index type `" + type + "` does not match the segment's vectors (" +
                                   (seg->binary ? "binary: BINARYMSTG, BINARYIVF" : "Float32: MSTG, IVFFLAT") + ")");
    if (btype) return build_binary_impl(seg, params);
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "metric_type", "nlist", "kmeans_iters", "sample", "plane"}, "index");
    int plane_fmt = MQVS_INDEX_PLANE_BF16;
    if (pm.count("plane")) {
        std::string pf = pm.at("plane");
        for (auto &ch : pf) ch = (char)std::tolower((unsigned char)ch);
        if (pf == "fp8")
            plane_fmt = MQVS_INDEX_PLANE_FP8;
        else if (pf != "bf16")
            fail(MQVS_ERR_BAD_ARGUMENTS, "index parameter `plane` = `" + pm.at("plane") + "` is not one of [bf16,fp8]");
    }
    int metric = seg->metric;
    if (pm.count("metric_type")) {
        std::string mt = pm.at("metric_type");
        for (auto &ch : mt) ch = (char)std::toupper((unsigned char)ch);
        if (mt == "L2")
            metric = MQVS_METRIC_L2;
        else if (mt == "IP")
            metric = MQVS_METRIC_IP;
        else if (mt == "COSINE")
            metric = MQVS_METRIC_COSINE;
        else
            fail(MQVS_ERR_NOT_IMPLEMENTED, "metric_type `" + pm.at("metric_type") + "` is not supported for Float32 vectors");
        if ((metric == MQVS_METRIC_COSINE) != (seg->metric == MQVS_METRIC_COSINE))
            fail(MQVS_ERR_LOGICAL, "segment was prepared for a different metric (cosine segments are normalised in HBM)");
    }
    const int64_t n = seg->n;
    const int d = seg->d;
    check_index_width(seg);
    if (!pm.count("nlist") && n >= kAutoNlistMinRows && !seg->nonempty_bits) return build_auto(seg, index_type, params);
    const BuildShape shape = build_shape(pm, n);
    return timed_build(seg, [&](mqvs_index *ix, hipStream_t s) {
        const int64_t S = shape.S;
        const int iters = shape.iters;
        ix->metric = metric;
        ix->coarse_metric = metric == MQVS_METRIC_L2 ? MQVS_METRIC_L2 : kMetricIpRaw;
        ix->nlist = shape.L;
        ix->alpha = shape.alpha;
        ix->dpad = round_up(d, kBfK);
        ix->plane_fmt = plane_fmt;
        const int cseg_metric = metric == MQVS_METRIC_L2 ? MQVS_METRIC_L2 : MQVS_METRIC_IP;

        // rows that can be indexed: non-empty arrays
        std::vector<uint8_t> keep;
        if (seg->nonempty_bits && n > 0) {
            std::vector<uint8_t> bits((n + 7) / 8);
            MQVS_HIP(hipMemcpyAsync(bits.data(), seg->nonempty_bits, bits.size(), hipMemcpyDeviceToHost, s));
            MQVS_HIP(hipStreamSynchronize(s));
            keep.resize(n);
            for (int64_t i = 0; i < n; ++i) keep[i] = (bits[i >> 3] >> (i & 7)) & 1;
        }

        // ---- k-means on a strided sample of the rows
        std::vector<int64_t> sidx;
        for (int64_t i = 0; i < S; ++i) {
            const int64_t r = (int64_t)((__int128)i * n / S);
            if (keep.empty() || keep[r]) sidx.push_back(r);
        }
        const int64_t Sm = (int64_t)sidx.size();
        const int64_t Lc = ix->nlist;
        TmpBuf dsidx(sizeof(int64_t) * std::max<int64_t>(Sm, 1));
        TmpBuf samp(sizeof(float) * std::max<int64_t>(Sm, 1) * d);
        TmpBuf cent(sizeof(float) * Lc * d);
        MQVS_HIP(hipMemsetAsync(cent.p, 0, sizeof(float) * Lc * d, s));
        if (Sm > 0) {
            MQVS_HIP(hipMemcpyAsync(dsidx.p, sidx.data(), sizeof(int64_t) * Sm, hipMemcpyHostToDevice, s));
            launch_gather_rows(seg->rows, d, d, dsidx.as<int64_t>(), Sm, samp.as<float>(), s);
            // initial centroids: evenly spaced sample rows
            std::vector<int64_t> init;
            for (int64_t c = 0; c < std::min(Lc, Sm); ++c) init.push_back((int64_t)((__int128)c * Sm / std::min(Lc, Sm)));
            TmpBuf dinit(sizeof(int64_t) * init.size());
            MQVS_HIP(hipMemcpyAsync(dinit.p, init.data(), sizeof(int64_t) * init.size(), hipMemcpyHostToDevice, s));
            launch_gather_rows(samp.as<float>(), d, d, dinit.as<int64_t>(), (int64_t)init.size(), cent.as<float>(), s);
            MQVS_HIP(hipGetLastError());
            MQVS_HIP(hipStreamSynchronize(s));
        }
        TmpBuf assign(sizeof(int64_t) * std::max<int64_t>(std::max(Sm, n), 1));
        TmpBuf adist(sizeof(float) * 8192);
        std::vector<int64_t> ha;
        std::vector<int32_t> order;
        std::vector<int64_t> off;
        for (int it = 0; it < iters && Sm > 0 && Lc > 1; ++it) {
            mqvs_segment *cs = segment_from_device(cent.as<float>(), Lc, d, cseg_metric, s);
            try {
                assign_rows(ix, cs, samp.as<float>(), Sm, assign.as<int64_t>(), adist.as<float>(), s);
            } catch (...) {
                segment_release(cs);
                throw;
            }
            segment_release(cs);
            ha.resize(Sm);
            MQVS_HIP(hipMemcpyAsync(ha.data(), assign.p, sizeof(int64_t) * Sm, hipMemcpyDeviceToHost, s));
            MQVS_HIP(hipStreamSynchronize(s));
            group_by_list(ha, Lc, 1, order, off);
            TmpBuf dord(sizeof(int32_t) * std::max<size_t>(order.size(), 1));
            TmpBuf doff(sizeof(int64_t) * off.size());
            if (!order.empty())
                MQVS_HIP(hipMemcpyAsync(dord.p, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, s));
            MQVS_HIP(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, s));
            launch_centroid_mean(samp.as<float>(), d, dord.as<int32_t>(), doff.as<int64_t>(), (int)Lc, cent.as<float>(), s);
            if (metric == MQVS_METRIC_COSINE) launch_normalize_rows(cent.as<float>(), Lc, d, s);
            MQVS_HIP(hipGetLastError());
            MQVS_HIP(hipStreamSynchronize(s));
        }
        ix->cent = segment_from_device(cent.as<float>(), Lc, d, cseg_metric, s);

        // ---- every row to its nearest centroid; lists in row order
        // a row no centroid can take (NaN components; an infinite one
        // whose product with every centroid is -inf or NaN) comes back
        // as -1: list 0 holds it, so every non-empty row is in a list
        // and a search of every list sees what FLAT sees (such a row can
        // still be a result: +inf under IP for a query of the other sign)
        TmpBuf canon(sizeof(int32_t) * std::max<int64_t>(n, 1));
        const bool assigned = Lc > 1 && n > 0;
        if (assigned) assign_rows(ix, ix->cent, seg->rows, n, assign.as<int64_t>(), adist.as<float>(), s);
        launch_grp_canon(assigned ? assign.as<int64_t>() : nullptr, n, Lc, seg->nonempty_bits, canon.as<int32_t>(), s);
        MQVS_HIP(hipGetLastError());
        finish_index(ix, canon.as<int32_t>(), false, s);
        ix->bytes += ix->cent->bytes;
    });
}

// ---- the list count from the data ------------------------------------------
// Without an explicit nlist, a part of at least 2^20 rows gets its list count
// from a sample: the fine default (about 256 rows per list) is built, and m =
// 1000 of the part's own rows are searched as queries against it at growing
// nprobe until recall@10 against their exact FLAT top-10 reaches 0.95.  If that
// takes more than 2 probes -- the data's clusters are larger than the lists,
// so a query's neighbours spread over many of them and every search pays the
// coarse step and plan of many small lists -- a coarse index (about 2048 rows
// per list) is built and evaluated the same way, and the faster of the two is
// kept (its recall-0.95 nprobe becomes alpha 3's).  The two are compared at
// the nprobe reaching recall 0.97 on the sample (0.95 if neither does): the
// sample's own rows are easier queries than held-out ones, and at 0.95 a
// borderline fine index (mode 2: 0.95 on the sample at nprobe 4, 0.9498 on
// held-out queries) won by a few per cent and then needed twice the probes in
// use.  The evaluation searches the index it built, so with plane=fp8 it
// measures the fp8 plane (the parameters are passed on to both builds).
// Data of many small clusters (generator mode 3) keeps the fine lists;
// data of few large ones (mode 2: 4096 centres over 10M rows) gets the coarse
// ones.
struct IndexEval {
    int nprobe = 0;  // recall 0.95 (0: not reached)
    int nprobe97 = 0;  // recall 0.97 (0: not reached)
    double ms = 1e30;  // a batch of the sample at nprobe97 (nprobe when 0.97 is not reached)
    double recall = 0.0;
};

// recall@10 of the sample's queries (rows of the part): the query row itself
// is dropped from both lists, so the figure is that of held-out queries
constexpr int kEvalK = 11;
// the timed searches of an operating point return the top-100 (a typical
// LIMIT: the re-rank and select then cost what they cost in use; timed at k =
// 11 the two list counts of a large-cluster part measured within a few per
// cent of each other, and the choice between them flipped with kernel changes)
constexpr int kEvalTimeK = 100;
static double sample_recall(const std::vector<int64_t> &got, const std::vector<int64_t> &gt,
                            const std::vector<int64_t> &self, int m) {
    int64_t hit = 0;
    for (int q = 0; q < m; ++q) {
        int64_t g[kEvalK], t[kEvalK];
        int ng = 0, nt = 0;
        for (int a = 0; a < kEvalK; ++a) {
            const int64_t x = got[(size_t)q * kEvalK + a], y = gt[(size_t)q * kEvalK + a];
            if (x != self[q] && ng < 10) g[ng++] = x;
            if (y != self[q] && nt < 10) t[nt++] = y;
        }
        for (int a = 0; a < ng; ++a)
            for (int b = 0; b < nt; ++b) hit += g[a] >= 0 && g[a] == t[b];
    }
    return (double)hit / (10.0 * m);
}

static IndexEval eval_index(mqvs_index *ix, const float *dq, int m, const std::vector<int64_t> &gt,
                            const std::vector<int64_t> &self, int64_t *dids, float *ddist, hipStream_t s) {
    IndexEval r;
    std::vector<int64_t> got((size_t)m * kEvalK);
    TimingEvent e0, e1;
    for (int np : {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64}) {
        if (np > std::min<int64_t>(ix->nlist, kSortCap)) break;
        const std::string sp = "nprobe=" + std::to_string(np);
        search_index_impl(ix, dq, m, kEvalK, sp.c_str(), nullptr, nullptr, dids, ddist, MQVS_F_DEVICE_PTRS, s, 0);
        MQVS_HIP(hipMemcpyAsync(got.data(), dids, sizeof(int64_t) * got.size(), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipStreamSynchronize(s));
        const double rc = sample_recall(got, gt, self, m);
        if (rc >= 0.95 && r.nprobe == 0) {
            r.nprobe = np;
            r.recall = rc;
        }
        if (rc >= 0.97) {
            r.nprobe97 = np;
            break;
        }
    }
    const int tnp = r.nprobe97 ? r.nprobe97 : r.nprobe;
    if (tnp > 0) {
        const std::string sp = "nprobe=" + std::to_string(tnp);
        for (int rep = 0; rep < 3; ++rep) {
            MQVS_HIP(hipEventRecord(e0.e, s));
            search_index_impl(ix, dq, m, (int)std::min<int64_t>(kEvalTimeK, ix->seg->n), sp.c_str(), nullptr,
                              nullptr, dids, ddist, MQVS_F_DEVICE_PTRS, s, 0);
            MQVS_HIP(hipEventRecord(e1.e, s));
            MQVS_HIP(hipStreamSynchronize(s));
            float ms = 0.f;
            MQVS_HIP(hipEventElapsedTime(&ms, e0.e, e1.e));
            r.ms = std::min(r.ms, (double)ms);
        }
    }
    return r;
}

static mqvs_index *build_auto(mqvs_segment *seg, const char *index_type, const char *params) {
    const int64_t n = seg->n;
    const int d = seg->d;
    const std::string base = params ? std::string(params) : std::string();
    auto with_nlist = [&](int64_t L) { return (base.empty() ? "" : base + ",") + "nlist=" + std::to_string(L); };
    const int64_t fine = std::max<int64_t>(1, std::min<int64_t>(65536, (n + 128) / 256));
    const int64_t coarse = std::max<int64_t>(1, (n + 1024) / 2048);
    const auto t0 = std::chrono::steady_clock::now();
    mqvs_index *a = build_impl(seg, index_type, with_nlist(fine).c_str());
    mqvs_index *b = nullptr;
    try {
        DeviceGuard guard(seg->device);
        hipStream_t s = thread_stream(seg->device);
        // the sample: m evenly spaced rows of the part as queries, their exact
        // FLAT top-10 as ground truth (the index's metric)
        const int m = (int)std::min<int64_t>(1000, n);
        std::vector<int64_t> idx(m);
        for (int i = 0; i < m; ++i) idx[i] = (int64_t)(((__int128)(2 * i + 1) * n) / (2 * m));
        TmpBuf didx(sizeof(int64_t) * m), dq(sizeof(float) * (size_t)m * d),
            dids(sizeof(int64_t) * (size_t)m * kEvalTimeK), ddist(sizeof(float) * (size_t)m * kEvalTimeK);
        MQVS_HIP(hipMemcpyAsync(didx.p, idx.data(), sizeof(int64_t) * m, hipMemcpyHostToDevice, s));
        launch_gather_rows(seg->rows, d, d, didx.as<int64_t>(), m, dq.as<float>(), s);
        MQVS_HIP(hipGetLastError());
        search_internal(seg, dq.as<float>(), m, kEvalK, a->metric, nullptr, nullptr, dids.as<int64_t>(),
                        ddist.as<float>(), MQVS_F_DEVICE_PTRS, s);
        std::vector<int64_t> gt((size_t)m * kEvalK);
        MQVS_HIP(hipMemcpyAsync(gt.data(), dids.p, sizeof(int64_t) * gt.size(), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipStreamSynchronize(s));
        std::vector<int64_t> self(m);
        for (int i = 0; i < m; ++i) self[i] = seg->row_offset + idx[i];
        const IndexEval ea = eval_index(a, dq.as<float>(), m, gt, self, dids.as<int64_t>(), ddist.as<float>(), s);
        a->np95 = ea.nprobe;
        if ((ea.nprobe == 0 || ea.nprobe > 2) && coarse < fine) {
            b = build_impl(seg, index_type, with_nlist(coarse).c_str());
            const IndexEval eb = eval_index(b, dq.as<float>(), m, gt, self, dids.as<int64_t>(), ddist.as<float>(), s);
            b->np95 = eb.nprobe;
            // (times are comparable only at the same target: an index that
            // reaches 0.97 within 64 probes beats one that does not.  The
            // coarse lists win ties within 15 %: the sample's timing is noisy
            // -- under a counter profiler the build once kept the fine lists --
            // and fewer lists keep the coarse step and the plan cheap at any
            // batch size)
            const bool a97 = ea.nprobe97 > 0, b97 = eb.nprobe97 > 0;
            const bool b_better = a97 != b97 ? b97 : (eb.nprobe > 0 && eb.ms < 1.15 * ea.ms);
            if (b_better) std::swap(a, b);
            free_index(b);
            b = nullptr;
        }
        // (the build time of the chosen index covers both builds and the sample)
        a->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) {
        free_index(a);
        if (b) free_index(b);
        throw;
    }
    return a;
}

// ---- binary index (BINARYMSTG seam) -------------------------------------------
// The reference's index over FixedString(N) columns (KAT 00038); MSTG's code
// is absent, so this is the library's own design: an inverted file over
// k-majority (Hamming k-means) lists, kernels_bivf.hip.  Binary distances are
// exact integers (Jaccard: one fp32 division of two integers), so the list
// scan computes the final distance and the search has no approximate stage:
// every returned distance equals mqvs_search_binary's on the same row, and a
// search that probes every list equals mqvs_search_binary bit for bit.
//
// Build (deterministic: integer arithmetic only).  The coarse metric is
// Hamming for both index metrics.  Sample rows floor(i n / S), initial
// centroids sample rows floor(c S / L); per iteration every sample row goes
// to the centroid at the smallest Hamming distance (ties: lowest list id) and
// each centroid bit becomes the majority of its members (2 ones > members; a
// list with no members keeps its centroid).  Every row is then assigned by
// the same rule and the codes are copied grouped by list, ascending row
// within a list.
int binary_metric_of(const std::string &name, const char *what) {
    std::string mt = name;
    for (auto &ch : mt) ch = (char)std::toupper((unsigned char)ch);
    if (mt == "HAMMING") return MQVS_METRIC_HAMMING;
    if (mt == "JACCARD") return MQVS_METRIC_JACCARD;
    fail(MQVS_ERR_NOT_IMPLEMENTED, std::string(what) + " `" + name + "` is not supported for binary vectors");
}

static mqvs_index *build_binary_impl(mqvs_segment *seg, const char *params) {
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "metric_type", "nlist", "kmeans_iters", "sample", "assign"}, "index");
    // assign: the kernel of the two assignment passes, valu (k_bivf_assign,
    // the default) or mfma (k_bivf_assign_mfma); the lists are the same
    const std::string assign_kind = pm.count("assign") ? pm.at("assign") : "valu";
    if (assign_kind != "valu" && assign_kind != "mfma")
        fail(MQVS_ERR_BAD_ARGUMENTS, "index parameter assign `" + assign_kind + "` is not valu or mfma");
    const bool assign_mfma = assign_kind == "mfma";
    if (assign_mfma && (int64_t)seg->code_words * 32 >= (1 << 24))
        fail(MQVS_ERR_NOT_IMPLEMENTED, "assign=mfma over codes of 2^24 or more bits");
    const int metric = pm.count("metric_type") ? binary_metric_of(pm.at("metric_type"), "metric_type") : seg->metric;
    const int64_t n = seg->n;
    if (n >= ((int64_t)1 << 31)) fail(MQVS_ERR_NOT_IMPLEMENTED, "binary index over 2^31 or more rows");
    const int cw = seg->code_words;
    const BuildShape shape = build_shape(pm, n);
    return timed_build(seg, [&](mqvs_index *ix, hipStream_t s) {
        const int64_t L = shape.L, S = shape.S;
        const int iters = shape.iters;
        ix->binary = true;
        ix->metric = metric;
        ix->coarse_metric = MQVS_METRIC_HAMMING;
        ix->nlist = L;
        ix->alpha = shape.alpha;
        ix->bcent = dalloc<uint32_t>(ix, (size_t)L * cw);
        MQVS_HIP(hipMemsetAsync(ix->bcent, 0, sizeof(uint32_t) * (size_t)L * cw, s));
        TmpBuf assign(sizeof(int32_t) * std::max<int64_t>(n, 1));
        // assign=mfma: the centroids as 0/1 bytes and their popcounts, expanded again by every pass
        TmpBuf cplane(assign_mfma ? bin_plane_bytes(L, cw) : 0), cpop(assign_mfma ? sizeof(uint32_t) * round_up(L, 16) : 0);
        auto assign_rows = [&](const uint32_t *codes, int64_t m) {
            if (assign_mfma)
                launch_bivf_assign_mfma(codes, m, cw, ix->bcent, (int)L, cplane.as<uint8_t>(), cpop.as<uint32_t>(),
                                        assign.as<int32_t>(), s);
            else
                launch_bivf_assign(codes, m, cw, ix->bcent, (int)L, assign.as<int32_t>(), s);
        };
        if (S > 0) {
            // ---- k-majority on a strided sample of the rows
            std::vector<int32_t> sidx(S);
            for (int64_t i = 0; i < S; ++i) sidx[i] = (int32_t)((__int128)i * n / S);
            const int64_t Li = std::min(L, S);
            std::vector<int32_t> init(Li);
            for (int64_t c = 0; c < Li; ++c) init[c] = (int32_t)((__int128)c * S / Li);
            TmpBuf didx(sizeof(int32_t) * S), dinit(sizeof(int32_t) * Li), samp(sizeof(uint32_t) * (size_t)S * cw);
            MQVS_HIP(hipMemcpyAsync(didx.p, sidx.data(), sizeof(int32_t) * S, hipMemcpyHostToDevice, s));
            MQVS_HIP(hipMemcpyAsync(dinit.p, init.data(), sizeof(int32_t) * Li, hipMemcpyHostToDevice, s));
            launch_bivf_gather(seg->codes, cw, didx.as<int32_t>(), S, samp.as<uint32_t>(), s);
            launch_bivf_gather(samp.as<uint32_t>(), cw, dinit.as<int32_t>(), Li, ix->bcent, s);
            MQVS_HIP(hipGetLastError());
            TmpBuf counts(sizeof(uint32_t) * (size_t)L * cw * 32), members(sizeof(uint32_t) * L);
            for (int it = 0; it < iters; ++it) {
                assign_rows(samp.as<uint32_t>(), S);
                MQVS_HIP(hipMemsetAsync(counts.p, 0, sizeof(uint32_t) * (size_t)L * cw * 32, s));
                MQVS_HIP(hipMemsetAsync(members.p, 0, sizeof(uint32_t) * L, s));
                launch_bivf_majority(samp.as<uint32_t>(), S, cw, assign.as<int32_t>(), (int)L, counts.as<uint32_t>(),
                                     members.as<uint32_t>(), ix->bcent, s);
                MQVS_HIP(hipGetLastError());
            }
            MQVS_HIP(hipStreamSynchronize(s));  // (sidx / init are host temporaries)
        }
        // ---- every row to its nearest centroid; lists in row order
        if (n > 0) {
            assign_rows(seg->codes, n);
            MQVS_HIP(hipGetLastError());
        }
        finish_index(ix, assign.as<int32_t>(), false, s);
    });
}

}  // namespace mqvs
