// index.hip -- the index path of libmqvs: an MSTG-type vector index over a
// resident segment (mqvs_index_*; C-ABI in include/mqvs.h).
//
// Reference seam (src/VectorIndex/Common/VIWithDataPart.cpp):
//   createIndex -> Search::createVectorIndex<..., FloatVector>(...)   :416-447
//   VIWithColumnInPart::search -> VectorIndex::search(queries, k, params,
//       first_stage_only, filter ∩ delete bitmap)                    :858-957
//   computeTopDistanceSubset (two-stage search, stage 2)              :838-856
// The MSTG library itself is absent from the snapshot, so the
// structure below is this library's own design for HBM and MFMA:
//
// Build (all on the GPU except the sample's counting sort per k-means step):
//   k-means over a row sample: assignment = FLAT top-1 search of the sample
//   rows against a centroid segment (the MFMA pre-filter path of mqvs_search),
//   deterministic ordered means (k_centroid_mean); cosine centroids are
//   re-normalised (spherical k-means).  Every row is then assigned to its
//   nearest centroid; finish_index groups the rows by list on the device (row
//   order within a list) and writes the lists back to back as a bf16 plane.
// Save / load (mqvs_index_save, mqvs_index_load; index_blob.hip): centroids +
//   each row's list behind a 64-byte header; the load ends in the same
//   finish_index.
// Search of a float index: index_search.hip.  This file holds the build, the
// list count's auto-tuning, the binary index and the C glue; index_internal.h
// what the three files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <chrono>
#include <vector>

#include "index_internal.h"

namespace mqvs {
mqvs_segment *index_segment(mqvs_index *idx) { return idx ? idx->seg : nullptr; }
}  // namespace mqvs

namespace mqvs {

thread_local mqvs_index_search_stats g_istats{};

static thread_local std::map<int, IndexWorkspace> *g_iws = nullptr;

// mqvs_thread_release: the calling thread's index workspaces (scratch,
// events, side stream, pinned words)
void index_thread_release() {
    if (!g_iws) return;
    for (auto &kv : *g_iws) {
        (void)hipSetDevice(kv.first);
        ws_detach_ext(kv.first, &kv.second);
        kv.second.release();
    }
    g_iws->clear();
}

IndexWorkspace &index_workspace(int device) {
    if (!g_iws) g_iws = new std::map<int, IndexWorkspace>();  // leaked at exit on purpose
    IndexWorkspace &w = (*g_iws)[device];
    w.init();
    return w;
}


// ---- Search::Parameters: "k=v,k=v" ----------------------------------------
std::map<std::string, std::string> parse_params(const char *s) {
    std::map<std::string, std::string> out;
    if (!s) return out;
    std::string str(s);
    size_t i = 0;
    while (i < str.size()) {
        size_t j = str.find(',', i);
        if (j == std::string::npos) j = str.size();
        std::string kv = str.substr(i, j - i);
        i = j + 1;
        auto trim = [](std::string x) {
            const auto b = x.find_first_not_of(" \t'\"");
            const auto e = x.find_last_not_of(" \t'\"");
            return b == std::string::npos ? std::string() : x.substr(b, e - b + 1);
        };
        kv = trim(kv);
        if (kv.empty()) continue;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) fail(MQVS_ERR_BAD_ARGUMENTS, "index parameter `" + kv + "` is not key=value");
        std::string key = trim(kv.substr(0, eq)), val = trim(kv.substr(eq + 1));
        for (auto &ch : key) ch = (char)std::tolower((unsigned char)ch);
        out[key] = val;
    }
    return out;
}

double num_param(const std::map<std::string, std::string> &m, const std::string &key, double dflt,
                        double lo, double hi) {
    auto it = m.find(key);
    if (it == m.end()) return dflt;
    char *end = nullptr;
    const double v = std::strtod(it->second.c_str(), &end);
    if (!end || *end != '\0' || it->second.empty() || !(v >= lo && v <= hi))
        fail(MQVS_ERR_BAD_ARGUMENTS, "index parameter `" + key + "` = `" + it->second + "` out of range [" +
                                         std::to_string(lo) + ", " + std::to_string(hi) + "]");
    return v;
}

void check_keys(const std::map<std::string, std::string> &m, const std::vector<std::string> &valid,
                       const char *what) {
    for (auto &kv : m) {
        if (std::find(valid.begin(), valid.end(), kv.first) == valid.end()) {
            std::string list;
            for (auto &v : valid) list += (list.empty() ? "" : ",") + v;
            fail(MQVS_ERR_BAD_ARGUMENTS, std::string("MSTG doesn't support ") + what + " parameter: `" + kv.first +
                                             "`, valid parameters is [" + list + "].");
        }
    }
}

// nprobe for a search alpha: nprobe(3) = base, doubling per unit of alpha;
// the base probes 1/256 of the lists and at least 4 lists and 4096 rows
int nprobe_of(const mqvs_index *ix, double alpha) {
    const double rows = (double)std::max<int64_t>(ix->rows_indexed, 1);
    // (an index whose list count was chosen from its data knows the nprobe
    // that reached recall@10 0.95 on the build's sample: alpha 3 probes 1.5x
    // that, a margin for queries unlike the part's own rows)
    const double base = ix->np95 > 0 ? (double)(ix->np95 + std::max(1, ix->np95 / 2))
                                     : std::max({4.0, std::ceil((double)ix->nlist / 256.0),
                                                 std::ceil(4096.0 * ix->nlist / rows)});
    const double np = std::ceil(base * std::pow(2.0, alpha - 3.0));
    return (int)std::max<double>(1.0, std::min<double>(np, (double)std::min<int64_t>(ix->nlist, kSortCap)));
}

// ---- build ------------------------------------------------------------------

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

void free_index(mqvs_index *ix) {
    if (!ix) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (ix->seg) (void)hipSetDevice(ix->seg->device);
    if (ix->cent) segment_release(ix->cent);
    for (void *q : {(void *)ix->plane, (void *)ix->perm, (void *)ix->pnorm, (void *)ix->list_off, (void *)ix->cplane,
                    (void *)ix->cperm, (void *)ix->cpnorm, (void *)ix->clist_off, (void *)ix->row_ids_map,
                    (void *)ix->yrec, (void *)ix->bplane, (void *)ix->bcent, (void *)ix->plane8,
                    (void *)ix->pscale})
        if (q) (void)hipFree(q);
    if (cur >= 0) (void)hipSetDevice(cur);
    delete ix;
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
// the device (kernels_ivf.hip: k_grp_*), then everything derived from that:
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

static mqvs_index *build_impl(mqvs_segment *seg, const char *index_type, const char *params) {
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
    // lists of about 256 rows (at most 65536 lists): fine enough that data of
    // many small clusters (generator mode 3: 65536 centres of ~150 rows)
    // keeps its neighbours in one or two lists; n / 1000 left mode 3 needing
    // 512 of 10000 lists for recall 0.95 (profiles/r03/index)
    const int64_t dflt_nlist = std::max<int64_t>(1, std::min<int64_t>(65536, (n + 128) / 256));
    const int64_t L = (int64_t)num_param(pm, "nlist", (double)dflt_nlist, 1, 1 << 20);
    if (n > 0 && L > n) fail(MQVS_ERR_BAD_ARGUMENTS, "nlist must not exceed the number of rows");
    const int iters = (int)num_param(pm, "kmeans_iters", 8, 0, 1000);
    // training sample: 64 rows per list up to 1M rows, at least 16 per list
    // (65536 lists: 1M rows, build 9.7 -> 4.1 s at equal recall, profiles/r03/index)
    const int64_t dflt_sample = std::min<int64_t>(n, std::max<int64_t>(16 * L, std::min<int64_t>(64 * L, 1 << 20)));
    const int64_t S = std::max<int64_t>(std::min<int64_t>(n, (int64_t)num_param(pm, "sample", (double)dflt_sample,
                                                                                 1, 1e12)),
                                        std::min<int64_t>(n, L));

    DeviceGuard guard(seg->device);
    hipStream_t s = thread_stream(seg->device);
    hipEvent_t e0, e1;
    MQVS_HIP(hipEventCreate(&e0));
    MQVS_HIP(hipEventCreate(&e1));
    MQVS_HIP(hipEventRecord(e0, s));

    auto *ix = new mqvs_index();
    try {
        ix->seg = seg;
        ix->metric = metric;
        ix->coarse_metric = metric == MQVS_METRIC_L2 ? MQVS_METRIC_L2 : kMetricIpRaw;
        ix->nlist = std::max<int64_t>(L, 1);
        ix->alpha = (float)num_param(pm, "alpha", 3.0, 1.0, 4.0);
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
        MQVS_HIP(hipEventRecord(e1, s));
        MQVS_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        MQVS_HIP(hipEventElapsedTime(&ms, e0, e1));
        ix->build_ms = ms;
        ix->bytes += ix->cent->bytes;
    } catch (...) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        free_index(ix);
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ix;
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
    hipEvent_t e0, e1;
    MQVS_HIP(hipEventCreate(&e0));
    MQVS_HIP(hipEventCreate(&e1));
    try {
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
                MQVS_HIP(hipEventRecord(e0, s));
                search_index_impl(ix, dq, m, (int)std::min<int64_t>(kEvalTimeK, ix->seg->n), sp.c_str(), nullptr,
                                  nullptr, dids, ddist, MQVS_F_DEVICE_PTRS, s, 0);
                MQVS_HIP(hipEventRecord(e1, s));
                MQVS_HIP(hipStreamSynchronize(s));
                float ms = 0.f;
                MQVS_HIP(hipEventElapsedTime(&ms, e0, e1));
                r.ms = std::min(r.ms, (double)ms);
            }
        }
    } catch (...) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
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
static int binary_metric_of(const std::string &name, const char *what) {
    std::string mt = name;
    for (auto &ch : mt) ch = (char)std::toupper((unsigned char)ch);
    if (mt == "HAMMING") return MQVS_METRIC_HAMMING;
    if (mt == "JACCARD") return MQVS_METRIC_JACCARD;
    fail(MQVS_ERR_NOT_IMPLEMENTED, std::string(what) + " `" + name + "` is not supported for binary vectors");
}

static mqvs_index *build_binary_impl(mqvs_segment *seg, const char *params) {
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "metric_type", "nlist", "kmeans_iters", "sample"}, "index");
    const int metric = pm.count("metric_type") ? binary_metric_of(pm.at("metric_type"), "metric_type") : seg->metric;
    const int64_t n = seg->n;
    if (n >= ((int64_t)1 << 31)) fail(MQVS_ERR_NOT_IMPLEMENTED, "binary index over 2^31 or more rows");
    const int cw = seg->code_words;
    const int64_t dflt_nlist = std::max<int64_t>(1, std::min<int64_t>(65536, (n + 128) / 256));
    const int64_t L = (int64_t)num_param(pm, "nlist", (double)dflt_nlist, 1, 1 << 20);
    if (n > 0 && L > n) fail(MQVS_ERR_BAD_ARGUMENTS, "nlist must not exceed the number of rows");
    const int iters = (int)num_param(pm, "kmeans_iters", 8, 0, 1000);
    const int64_t dflt_sample = std::min<int64_t>(n, std::max<int64_t>(16 * L, std::min<int64_t>(64 * L, 1 << 20)));
    const int64_t S = std::max<int64_t>(std::min<int64_t>(n, (int64_t)num_param(pm, "sample", (double)dflt_sample,
                                                                                 1, 1e12)),
                                        std::min<int64_t>(n, L));

    DeviceGuard guard(seg->device);
    hipStream_t s = thread_stream(seg->device);
    hipEvent_t e0, e1;
    MQVS_HIP(hipEventCreate(&e0));
    MQVS_HIP(hipEventCreate(&e1));
    MQVS_HIP(hipEventRecord(e0, s));
    auto *ix = new mqvs_index();
    try {
        ix->seg = seg;
        ix->binary = true;
        ix->metric = metric;
        ix->coarse_metric = MQVS_METRIC_HAMMING;
        ix->nlist = L;
        ix->alpha = (float)num_param(pm, "alpha", 3.0, 1.0, 4.0);
        ix->bcent = dalloc<uint32_t>(ix, (size_t)L * cw);
        MQVS_HIP(hipMemsetAsync(ix->bcent, 0, sizeof(uint32_t) * (size_t)L * cw, s));
        TmpBuf assign(sizeof(int32_t) * std::max<int64_t>(n, 1));
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
                launch_bivf_assign(samp.as<uint32_t>(), S, cw, ix->bcent, (int)L, assign.as<int32_t>(), s);
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
            launch_bivf_assign(seg->codes, n, cw, ix->bcent, (int)L, assign.as<int32_t>(), s);
            MQVS_HIP(hipGetLastError());
        }
        finish_index(ix, assign.as<int32_t>(), false, s);
        MQVS_HIP(hipEventRecord(e1, s));
        MQVS_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        MQVS_HIP(hipEventElapsedTime(&ms, e0, e1));
        ix->build_ms = ms;
    } catch (...) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        free_index(ix);
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ix;
}

// Search: the nprobe nearest centroids by (Hamming, list id) (every list, with
// no ranking, when nprobe == nlist), the probed lists scanned with the search
// metric, filter ∩ row_exists and the b < nBit rule applied per position, and
// the k best by (distance, part row) taken by the brute-force path's final
// select (which keeps the smallest rows of a tie group at the k-th key however
// large the group is).  probes_out (mqvs_index_probes_binary): the coarse
// step's probes[nq][nprobe] are copied there and the search ends.
static void search_binary_index_impl(mqvs_index *ix, const uint8_t *queries, int nq, int k, const char *params,
                                     const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                                     uint32_t flags, hipStream_t user_stream, int64_t *probes_out) {
    check_search_args(ix, "index", ix && !ix->binary ? "Float32 index: search it with mqvs_index_search" : nullptr, nq,
                      k, queries, out_ids, out_dist);
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "nprobe", "num_reorder", "metric"}, "search");
    const int metric = pm.count("metric") ? binary_metric_of(pm.at("metric"), "metric") : ix->metric;
    const double alpha = num_param(pm, "alpha", ix->alpha, 1.0, 4.0);
    const int nprobe = pm.count("nprobe")
                           ? (int)num_param(pm, "nprobe", 1, 1, (double)std::min<int64_t>(ix->nlist, kSortCap))
                           : nprobe_of(ix, alpha);
    // (accepted and ignored: the scan is exact, nothing is re-ordered)
    (void)num_param(pm, "num_reorder", 1, 1, (double)kLargeCap);
    mqvs_index_search_stats st{};
    st.nq = nq;
    st.k = k;
    st.nprobe = nprobe;
    g_istats = st;
    if (nq == 0 || k == 0) return;

    mqvs_segment *seg = ix->seg;
    const bool rank = nprobe < ix->nlist;
    // a query's records: at most every position of its probed lists
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>((int64_t)nprobe * ix->max_list, ix->npos));
    {
        // query sub-batches under the scratch budget (records, centroid
        // distances, the large-k sort scratch)
        const int64_t perq = cap * (int64_t)sizeof(Cand) + (rank ? ix->nlist * 4 : 0) +
                             (k > kSortCap ? (int64_t)sizeof(uint4) * 2 * kLargeCap : 0);
        const int qb = (int)std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)scratch_budget() / perq));
        if (nq > qb) {
            mqvs_index_search_stats sum{};
            for_query_batches(nq, qb, [&](int q0, int m) {
                search_binary_index_impl(ix, queries + (size_t)q0 * seg->code_bytes, m, k, params, filter, exists,
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
            sum.nq = nq;
            sum.k = k;
            sum.nprobe = nprobe;
            g_istats = sum;
            return;
        }
    }

    DeviceGuard guard(seg->device);
    IndexWorkspace &ws = index_workspace(seg->device);
    WsScope scope(seg->device, &ws);
    hipStream_t s = user_stream ? user_stream : thread_stream(seg->device);
    scope.set_stream(s);
    const bool dev = flags & MQVS_F_DEVICE_PTRS;
    const bool tev = timing_on(flags);
    const int cw = seg->code_words;
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[0], s));

    // queries -> zero-padded [nq][code_words]
    auto *qc = (uint32_t *)ws.io.queries.get(sizeof(uint32_t) * (size_t)nq * cw);
    upload_codes(qc, cw, queries, seg->code_bytes, nq, dev, s);
    const CallIO::In in = ws.io.in(nullptr, 0, filter, exists, (seg->n + 7) / 8, dev, s);
    const uint8_t *dfilter = in.filter, *dexists = in.exists;
    const CallIO::Out out = ws.io.out((size_t)nq * k, dev, out_ids, out_dist);
    int64_t *dids = out.ids;
    float *ddist = out.dist;
    // [0] the final select's overflow word (never set: a region holds every
    // position of its lists)
    int *status = (int *)ws.status.get(sizeof(int) * 8);
    int *count = (int *)ws.fine.lcount.get(sizeof(int) * nq);
    launch_fill2(reinterpret_cast<uint32_t *>(status), 8, 0u, reinterpret_cast<uint32_t *>(count), nq, 0u, s);

    // ---- coarse
    int64_t *probes = (int64_t *)ws.probes.get(sizeof(int64_t) * (size_t)nq * nprobe);
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
    if (probes_out) {
        MQVS_HIP(hipMemcpyAsync(probes_out, probes, sizeof(int64_t) * (size_t)nq * nprobe, hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipEventRecord(ws.ev[5], s));
        host_wait(s);
        return;
    }

    // ---- the probed lists
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
    p.cand = (Cand *)ws.fine.cand.get(sizeof(Cand) * (size_t)nq * cap);
    p.cand_count = count;
    p.cand_cap = (int)cap;
    int64_t *dstats = (int64_t *)ws.fine.stats.get(sizeof(int64_t) * 4);
    launch_bivf_scan(p, metric, dstats, s);
    MQVS_HIP(hipGetLastError());
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[3], s));
    uint4 *large = k > kSortCap ? (uint4 *)ws.fine.large.get(sizeof(uint4) * 2 * kLargeCap * (size_t)nq) : nullptr;
    // ascending finite values: the L2 ordering key, (key, row) ties
    launch_final_select(p.cand, count, (int)cap, nq, k, MQVS_METRIC_L2, 0, seg->row_offset, dids, ddist, status, large,
                        s);
    MQVS_HIP(hipGetLastError());
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[4], s));
    MQVS_HIP(hipEventRecord(ws.ev[5], s));

    // decoupled part: results in the new part's row ids
    if (ix->row_ids_map) launch_map_ids(dids, (int64_t)nq * k, ix->row_ids_map, s);
    if (dev && (flags & MQVS_F_ASYNC)) {
        launch_async_flags(status, nullptr, 0, async_sticky(seg->device, s), s);
        MQVS_HIP(hipGetLastError());
        return;
    }
    int64_t *hs = ws.host;
    int *hst = reinterpret_cast<int *>(ws.host + 4);
    ws.io.finish_begin(out, s);
    launch_words_to_host(dstats, 4, status, 8, hs, hst, s);
    MQVS_HIP(hipGetLastError());
    host_wait(s);
    if (*hst) fail(MQVS_ERR_DEVICE, "binary index search: a query's record region overflowed");
    ws.io.finish_end(out);
    st.values = hs[0];
    st.items = hs[1];
    st.plane_bytes = hs[2];
    st.pairs = hs[3];
    if (tev) {
        float t[4] = {0, 0, 0, 0}, tot = 0;
        for (int i = 0; i < 4; ++i) MQVS_HIP(hipEventElapsedTime(&t[i], ws.ev[i], ws.ev[i + 1]));
        MQVS_HIP(hipEventElapsedTime(&tot, ws.ev[0], ws.ev[5]));
        st.coarse_ms = t[0];
        st.scan_ms = t[2];
        st.select_ms = t[3];
        st.total_ms = tot;
    }
    g_istats = st;
}

}  // namespace mqvs

using namespace mqvs;

extern "C" {

int mqvs_index_build(mqvs_segment_t seg, const char *index_type, const char *params, mqvs_index_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        *out = build_impl(seg, index_type, params);
    });
}

int mqvs_index_free(mqvs_index_t idx) {
    return guarded([&] { free_index(idx); });
}

int mqvs_index_info(mqvs_index_t idx, mqvs_index_info_t *out) {
    return guarded([&] {
        if (!idx || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        out->nlist = idx->nlist;
        out->npos = idx->npos;
        out->max_list = idx->max_list;
        out->rows_indexed = idx->rows_indexed;
        out->metric = idx->metric;
        out->dim = idx->seg->d;
        out->hbm_bytes = idx->bytes;
        out->build_ms = idx->build_ms;
    });
}

int mqvs_index_plane(mqvs_index_t idx, int32_t *format, size_t *plane_bytes) {
    return guarded([&] {
        if (!idx) fail(MQVS_ERR_BAD_ARGUMENTS, "null index");
        if (idx->binary) fail(MQVS_ERR_LOGICAL, "binary index: it has no float list plane");
        const bool fp8 = idx->plane_fmt == MQVS_INDEX_PLANE_FP8;
        if (format) *format = idx->plane_fmt;
        if (plane_bytes)
            *plane_bytes = (size_t)idx->npos * (size_t)idx->dpad * (fp8 ? 1 : 2) +
                           (fp8 ? sizeof(int16_t) * (size_t)idx->npos : 0);
    });
}

int mqvs_index_search_ex(mqvs_index_t idx, const float *queries, int32_t nq, int32_t k, const char *params,
                         const uint8_t *filter, const uint8_t *row_exists, int64_t chunk_ord_base, int64_t *out_ids,
                         float *out_dist, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        if (chunk_ord_base > INT32_MAX) fail(MQVS_ERR_BAD_ARGUMENTS, "chunk_ord_base out of range");
        WaitScope wsc{4, (uint64_t)(uintptr_t)idx, (uint64_t)nq, (uint64_t)k, wait_str_hash(params), filter != nullptr,
                      row_exists != nullptr, flags};
        search_index_impl(idx, queries, nq, k, params, filter, row_exists, out_ids, out_dist, flags,
                          (hipStream_t)stream, 0, 0, chunk_ord_base);
    });
}

int mqvs_index_search(mqvs_index_t idx, const float *queries, int32_t nq, int32_t k, const char *params,
                      const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                      uint32_t flags, mqvs_stream_t stream) {
    return mqvs_index_search_ex(idx, queries, nq, k, params, filter, row_exists, -1, out_ids, out_dist, flags, stream);
}

int mqvs_index_centroids(mqvs_index_t idx, float *out, int64_t cap) {
    return guarded([&] {
        if (!idx || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (idx->binary) fail(MQVS_ERR_LOGICAL, "binary index: read its centroids with mqvs_index_centroids_binary");
        if (!idx->cent) fail(MQVS_ERR_LOGICAL, "index has no centroid table");
        const int64_t need = idx->cent->n * (int64_t)idx->cent->d;
        if (cap < need) fail(MQVS_ERR_BAD_ARGUMENTS, "output holds " + std::to_string(cap) + " floats, " +
                                                         std::to_string(need) + " needed");
        DeviceGuard guard(idx->cent->device);
        MQVS_HIP(hipMemcpy(out, idx->cent->rows, sizeof(float) * (size_t)need, hipMemcpyDeviceToHost));
    });
}

int mqvs_index_probes(mqvs_index_t idx, const float *queries, int32_t nq, const char *params, int64_t *out_probes) {
    return guarded([&] {
        if (!idx || (nq > 0 && (!queries || !out_probes))) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (nq < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "nq must be non-negative");
        if (nq == 0) return;
        struct Reset {
            ~Reset() { t_probes_out = nullptr; }
        } reset;
        t_probes_out = out_probes;
        WaitScope wsc{5, (uint64_t)(uintptr_t)idx, (uint64_t)nq, wait_str_hash(params)};
        // k 1: the coarse step does not depend on k; the search stops after it
        std::vector<int64_t> ids((size_t)nq);
        std::vector<float> dd((size_t)nq);
        search_index_impl(idx, queries, nq, 1, params, nullptr, nullptr, ids.data(), dd.data(), 0, nullptr, 0);
    });
}

int mqvs_index_search_binary(mqvs_index_t idx, const uint8_t *queries, int32_t nq, int32_t k, const char *params,
                             const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                             uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{6, (uint64_t)(uintptr_t)idx, (uint64_t)nq, (uint64_t)k, wait_str_hash(params), filter != nullptr,
                      row_exists != nullptr, flags};
        search_binary_index_impl(idx, queries, nq, k, params, filter, row_exists, out_ids, out_dist, flags,
                                 (hipStream_t)stream, nullptr);
    });
}

int mqvs_index_centroids_binary(mqvs_index_t idx, uint8_t *out, int64_t cap_bytes) {
    return guarded([&] {
        if (!idx || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (!idx->binary) fail(MQVS_ERR_LOGICAL, "Float32 index: read its centroids with mqvs_index_centroids");
        const int64_t nb = idx->seg->code_bytes;
        const int64_t need = idx->nlist * nb;
        if (cap_bytes < need) fail(MQVS_ERR_BAD_ARGUMENTS, "output holds " + std::to_string(cap_bytes) + " bytes, " +
                                                               std::to_string(need) + " needed");
        DeviceGuard guard(idx->seg->device);
        MQVS_HIP(hipMemcpy2D(out, (size_t)nb, idx->bcent, (size_t)idx->seg->code_words * 4, (size_t)nb,
                             (size_t)idx->nlist, hipMemcpyDeviceToHost));
    });
}

int mqvs_index_probes_binary(mqvs_index_t idx, const uint8_t *queries, int32_t nq, const char *params,
                             int64_t *out_probes) {
    return guarded([&] {
        if (!idx || (nq > 0 && (!queries || !out_probes))) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (nq < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "nq must be non-negative");
        if (nq == 0) return;
        WaitScope wsc{7, (uint64_t)(uintptr_t)idx, (uint64_t)nq, wait_str_hash(params)};
        // k 1: the coarse step does not depend on k; the search stops after it
        std::vector<int64_t> ids((size_t)nq);
        std::vector<float> dd((size_t)nq);
        search_binary_index_impl(idx, queries, nq, 1, params, nullptr, nullptr, ids.data(), dd.data(), 0, nullptr,
                                 out_probes);
    });
}

int mqvs_index_save_size(mqvs_index_t idx, size_t *bytes) {
    return guarded([&] {
        if (!idx || !bytes) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        *bytes = blob_bytes(idx);
    });
}

int mqvs_index_save(mqvs_index_t idx, uint8_t *out, size_t cap, size_t *written) {
    return guarded([&] {
        if (written) *written = 0;
        const size_t w = save_impl(idx, out, cap);
        if (written) *written = w;
    });
}

int mqvs_index_load(mqvs_segment_t seg, const uint8_t *blob, size_t bytes, mqvs_index_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        *out = load_impl(seg, blob, bytes);
    });
}

int mqvs_index_blob_info(const uint8_t *blob, size_t bytes, mqvs_index_blob_info_t *out) {
    return guarded([&] { blob_info_impl(blob, bytes, out); });
}

int mqvs_index_lists(mqvs_index_t idx, int64_t *list_off, int64_t cap_off, int32_t *rows, int64_t cap_rows) {
    return guarded([&] {
        if (!idx || !list_off || (idx->npos > 0 && !rows)) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (cap_off < idx->nlist + 1 || cap_rows < idx->npos)
            fail(MQVS_ERR_BAD_ARGUMENTS, "outputs hold " + std::to_string(cap_off) + " offsets and " +
                                             std::to_string(cap_rows) + " rows, " + std::to_string(idx->nlist + 1) +
                                             " and " + std::to_string(idx->npos) + " needed");
        DeviceGuard guard(idx->seg->device);
        MQVS_HIP(hipMemcpy(list_off, idx->list_off, sizeof(int64_t) * (size_t)(idx->nlist + 1), hipMemcpyDeviceToHost));
        if (idx->npos > 0)
            MQVS_HIP(hipMemcpy(rows, idx->perm, sizeof(int32_t) * (size_t)idx->npos, hipMemcpyDeviceToHost));
    });
}

int mqvs_index_set_row_ids_map(mqvs_index_t idx, const uint64_t *row_ids_map, int64_t len, uint32_t flags) {
    return guarded([&] {
        if (!idx) fail(MQVS_ERR_BAD_ARGUMENTS, "null index");
        DeviceGuard guard(idx->seg->device);
        if (idx->row_ids_map) {
            MQVS_HIP(hipFree(idx->row_ids_map));
            idx->bytes -= sizeof(uint64_t) * (size_t)idx->row_ids_len;
            idx->row_ids_map = nullptr;
            idx->row_ids_len = 0;
        }
        if (!row_ids_map || len <= 0) return;
        if (len < idx->seg->row_offset + idx->seg->n)
            fail(MQVS_ERR_BAD_ARGUMENTS, "row_ids_map shorter than the indexed part (" + std::to_string(len) + " < " +
                                             std::to_string(idx->seg->row_offset + idx->seg->n) + ")");
        uint64_t *m = nullptr;
        if (hipMalloc((void **)&m, sizeof(uint64_t) * (size_t)len) != hipSuccess) {
            (void)hipGetLastError();
            fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of the row id map failed");
        }
        MQVS_HIP(hipMemcpy(m, row_ids_map, sizeof(uint64_t) * (size_t)len,
                           (flags & MQVS_F_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        idx->row_ids_map = m;
        idx->row_ids_len = len;
        idx->bytes += sizeof(uint64_t) * (size_t)len;
    });
}

int mqvs_decoupled_filter(const uint8_t *new_filter, int64_t new_rows, const uint64_t *inverted_row_ids_map,
                          const uint8_t *inverted_row_sources_map, int64_t inverted_len, uint32_t own_id,
                          uint8_t *old_filter, int64_t old_rows, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        if (new_rows < 0 || old_rows < 0 || inverted_len < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if ((new_rows && !new_filter) || (old_rows && !old_filter))
            fail(MQVS_ERR_BAD_ARGUMENTS, "null bitmap");
        if (inverted_len > 0 && (!inverted_row_ids_map || !inverted_row_sources_map))
            fail(MQVS_ERR_BAD_ARGUMENTS, "null inverted map");
        int dev = 0;
        MQVS_HIP(hipGetDevice(&dev));
        IndexWorkspace &ws = index_workspace(dev);
        WsScope scope(dev, &ws);
        hipStream_t s = stream ? (hipStream_t)stream : thread_stream(dev);
        scope.set_stream(s);
        const bool devp = flags & MQVS_F_DEVICE_PTRS;
        const int64_t nb = (new_rows + 7) / 8, ob = (old_rows + 7) / 8;
        const uint8_t *df = new_filter;
        const uint64_t *dinv = inverted_row_ids_map;
        const uint8_t *dsrc = inverted_row_sources_map;
        if (!devp) {
            auto *b = (uint8_t *)ws.dmap.get((size_t)nb + 16 + (size_t)inverted_len * 9 + 16);
            MQVS_HIP(hipMemcpyAsync(b, new_filter, nb, hipMemcpyHostToDevice, s));
            df = b;
            auto *inv = (uint64_t *)(b + (nb + 15) / 16 * 16);
            if (inverted_len) {
                MQVS_HIP(hipMemcpyAsync(inv, inverted_row_ids_map, 8 * (size_t)inverted_len, hipMemcpyHostToDevice, s));
                MQVS_HIP(hipMemcpyAsync((uint8_t *)(inv + inverted_len), inverted_row_sources_map, inverted_len,
                                        hipMemcpyHostToDevice, s));
            }
            dinv = inv;
            dsrc = (const uint8_t *)(inv + inverted_len);
        }
        auto *words = (uint32_t *)ws.dwords.get(4 * (size_t)((old_rows + 31) / 32) + 16);
        launch_decoupled_filter(df, new_rows, inverted_len ? dinv : nullptr, dsrc, inverted_len, own_id, words,
                                old_rows, s);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(old_filter, words, ob, devp ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        if (!(devp && (flags & MQVS_F_ASYNC))) host_wait(s);
    });
}

int mqvs_index_last_stats(mqvs_index_search_stats *out) {
    if (!out) return MQVS_ERR_BAD_ARGUMENTS;
    *out = g_istats;
    return MQVS_OK;
}

}  // extern "C"
