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
// Save / load (mqvs_index_save, mqvs_index_load): centroids + each row's list
//   behind a 64-byte header; the load ends in the same finish_index.
// Search:
//   coarse   FLAT search of the queries against the centroid segment, k =
//            nprobe (L2 for L2 parts, raw inner product for IP and cosine)
//   plan     (query, list) pairs grouped by list into 16-query work items
//   scan     bf16 MFMA over each probed list (kernels_ivf.hip); an index built
//            with plane=fp8 keeps e4m3fn codes there, widened in registers
//   select   num_reorder best approximate values per query
//   re-rank  exact fp32 distances of those rows (k_rerank_ids: the formula
//            and cosine query variant of mqvs_search / mqvs_rerank), top-k by
//            the reference order key
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <chrono>
#include <vector>

#include "mqvs_internal.h"

struct mqvs_index {
    mqvs_segment *seg = nullptr;   // borrowed: the caller keeps the segment alive
    int metric = 0;                // search metric (L2, IP or Cosine)
    int coarse_metric = 0;         // L2 or kMetricIpRaw
    int64_t nlist = 0;
    int64_t npos = 0;
    int64_t max_list = 0;
    int64_t rows_indexed = 0;
    int64_t dpad = 0;
    float alpha = 3.0f;            // default search alpha
    mqvs_segment *cent = nullptr;  // centroid segment (k-means assignment during the build)
    uint16_t *plane = nullptr;     // bf16 rows in list order, [npos/16][dpad/32][16][32] (k_ivf_pack)
    // plane=fp8 (plane_fmt MQVS_INDEX_PLANE_FP8; `plane` is then null): e4m3fn
    // codes in list order, [npos/16][dpad/64][16][64], and each position's
    // scale exponent (k_to_fp8)
    int plane_fmt = MQVS_INDEX_PLANE_BF16;
    uint8_t *plane8 = nullptr;
    int16_t *pscale = nullptr;
    int32_t *perm = nullptr;       // [npos] row of each position, -1 = padding
    float *pnorm = nullptr;        // [npos] |y|^2
    int64_t *list_off = nullptr;   // [nlist+1]
    float *yrec = nullptr;         // [kMxRec] maxima over the rows of |bf16(y)|, |y - bf16(y)|, |y| (the
                                   // re-rank's bound pruning: k_query_bound's segment record; fp8: of
                                   // the de-scaled codes, over the indexed positions)
    // coarse quantizer in the same list layout: the centroids in chunks of
    // kCoarseChunk (every query probes every chunk), bf16 plane + |c|^2
    int64_t cnl = 0, cnpos = 0, cmax = 0;
    uint16_t *cplane = nullptr;
    int32_t *cperm = nullptr;
    float *cpnorm = nullptr;
    int64_t *clist_off = nullptr;
    // decoupled part (VIWithMeta::row_ids_map): old part row -> row id in the
    // decoupled part, applied to every result (transferToNewRowIds)
    uint64_t *row_ids_map = nullptr;
    int64_t row_ids_len = 0;
    size_t bytes = 0;
    double build_ms = 0.0;
    int np95 = 0;                  // nprobe measured to reach recall@10 0.95 on the build's sample (0: not measured)
    // binary index (BINARYMSTG; kernels_bivf.hip): metric is Hamming or
    // Jaccard, perm / list_off as above (no padding positions)
    bool binary = false;
    uint32_t *bplane = nullptr;    // [npos][code_words] codes in list order
    uint32_t *bcent = nullptr;     // [nlist][code_words] k-majority centroids
};

namespace mqvs {
mqvs_segment *index_segment(mqvs_index *idx) { return idx ? idx->seg : nullptr; }
}  // namespace mqvs

namespace mqvs {

static thread_local mqvs_index_search_stats g_istats{};
constexpr int64_t kCoarseChunk = 256;  // centroids per coarse "list"
constexpr int64_t kCoarseFlatLists = 16384;  // more lists: the coarse step is a FLAT search

// plan / scan / select buffers of one list pass
struct ListBufs {
    GBuf lcount, lfill, lstart, lq, items, grp, chk, nitems, qbase, qstart, cand, stats, large;
    size_t release() {
        size_t b = 0;
        for (GBuf *x : {&lcount, &lfill, &lstart, &lq, &items, &grp, &chk, &nitems, &qbase, &qstart, &cand, &stats,
                        &large}) {
            b += x->cap;
            x->release();
        }
        return b;
    }
};

// The scratch of a thread's index searches.  Every buffer is a GBuf: it grows
// through the thread's FLAT workspace gate (WsScope in search_index_impl), so
// concurrent index searches share the process-wide HBM budget with FLAT
// scans, and an idle thread's index scratch is trimmed with its workspace.
struct IndexWorkspace final : WsExt {
    hipEvent_t ev[6] = {};
    // the cosine variant chain runs on `side` between fork and join (created
    // on the workspace's device: index_workspace is called under its guard)
    hipEvent_t fork = nullptr, join = nullptr;
    hipStream_t side = nullptr;
    int64_t *host = nullptr;  // pinned: the search's stats [4] and status word (one sync, no staging copies)
    CallIO io;  // staged inputs and outputs of host-pointer searches
    GBuf qvars, qnorms, qmu, qlam, status, qhi, probes, cprobes, rows, ord, dmap, dwords, pdist, cqhi, gmax, crec, cbq,
        craw, ibq, qdelta, pstats, q8, q8exp, q8rec;
    ListBufs coarse, fine;
    // WsExt: the owner is between calls (its workspace's `done` event passed:
    // the main stream, which joins the side chain, has drained)
    size_t free_scratch() override {
        if (side) (void)hipStreamSynchronize(side);
        size_t b = io.release();
        for (GBuf *x : {&qvars, &qnorms, &qmu, &qlam, &status, &qhi, &probes, &cprobes, &rows, &ord, &dmap, &dwords,
                        &pdist, &cqhi, &gmax, &crec, &cbq, &craw, &ibq, &qdelta, &pstats, &q8, &q8exp, &q8rec}) {
            b += x->cap;
            x->release();
        }
        return b + coarse.release() + fine.release();
    }
    void init() {
        if (ev[0]) return;
        for (auto &e : ev) MQVS_HIP(hipEventCreate(&e));
        MQVS_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
        MQVS_HIP(hipEventCreateWithFlags(&join, hipEventDisableTiming));
        MQVS_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        MQVS_HIP(hipHostMalloc((void **)&host, 8 * sizeof(int64_t), hipHostMallocDefault));
    }
    // after the last search's kernels (ev[5] ends every search, ASYNC ones
    // included; the side stream's chain is joined before it)
    // (the scratch is detached and freed first: ws_detach_ext)
    void release() {
        if (!ev[0]) return;
        (void)hipEventSynchronize(ev[5]);
        if (side) (void)hipStreamSynchronize(side);
        for (auto &e : ev) {
            (void)hipEventDestroy(e);
            e = nullptr;
        }
        (void)hipEventDestroy(fork);
        (void)hipEventDestroy(join);
        (void)hipStreamDestroy(side);
        (void)hipHostFree(host);
        fork = join = nullptr;
        side = nullptr;
        host = nullptr;
    }
};

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

static IndexWorkspace &index_workspace(int device) {
    if (!g_iws) g_iws = new std::map<int, IndexWorkspace>();  // leaked at exit on purpose
    IndexWorkspace &w = (*g_iws)[device];
    w.init();
    return w;
}


// ---- Search::Parameters: "k=v,k=v" ----------------------------------------
static std::map<std::string, std::string> parse_params(const char *s) {
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

static double num_param(const std::map<std::string, std::string> &m, const std::string &key, double dflt,
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

static void check_keys(const std::map<std::string, std::string> &m, const std::vector<std::string> &valid,
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
static int nprobe_of(const mqvs_index *ix, double alpha) {
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

static void free_index(mqvs_index *ix) {
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

template <typename T>
static T *dalloc(mqvs_index *ix, size_t count) {
    T *p = nullptr;
    const size_t bytes = sizeof(T) * std::max<size_t>(count, 1);
    if (hipMalloc((void **)&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of " + std::to_string(bytes) + " bytes failed");
    }
    ix->bytes += bytes;
    return p;
}

struct TmpBuf {
    void *p = nullptr;
    explicit TmpBuf(size_t bytes) {
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) {
            (void)hipGetLastError();
            fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of " + std::to_string(bytes) + " bytes failed");
        }
    }
    ~TmpBuf() {
        if (p) (void)hipFree(p);
    }
    template <typename T>
    T *as() const {
        return (T *)p;
    }
};

static void search_index_impl(mqvs_index *ix, const float *queries, int nq, int k, const char *params,
                              const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                              uint32_t flags, hipStream_t user_stream, int formula_nq, int maxv_hint = 0);
static mqvs_index *build_auto(mqvs_segment *seg, const char *index_type, const char *params);
constexpr int64_t kAutoNlistMinRows = 1 << 20;  // smaller parts take the default list count

static mqvs_index *build_binary_impl(mqvs_segment *seg, const char *params);

// the list scan keeps a tile of at least 16 bf16 queries in LDS
// (ivf_scan_lds): rows too wide for that cannot be searched
static void check_index_width(mqvs_segment *seg) {
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
static void finish_index(mqvs_index *ix, const int32_t *assign, bool from_blob, hipStream_t s) {
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

// ---- search -----------------------------------------------------------------

// One list pass: plan + bf16 MFMA scan + select of nq queries over a list
// layout (the index's lists, or the coarse quantizer's centroid chunks).
// probes[nq][nprobe] are list ids; out: the R best rows per query by the
// approximate distance (+ id_offset; with out_approx, ids and approximate
// distances for a first-stage result).  ev (optional): events 2..4 after
// plan, scan and select.  pair_stats ([nq][4] words; null: no pair mode):
// few pairs per list take pair mode (no plan; the select writes each query's
// stats there).  Returns the stats words of the pass; *per_query: whether
// they are pair mode's per-query rows.  f8 (an fp8 index's fine pass): the
// plane's codes and scale exponents and the queries' exponents; `plane` is
// unused and qhi holds the queries' scaled codes as bf16 values.
struct ListFp8 {
    const uint8_t *plane8;
    const int16_t *pscale;
    const int16_t *qexp;
};
static int64_t *list_pass(ListBufs &b, const uint16_t *plane, const int32_t *perm, const float *pnorm,
                          const int64_t *list_off, int64_t nlist, int64_t npos, int64_t max_list, int64_t dpad,
                          int metric, const uint16_t *qhi, const float *qnorm, int nq, const int64_t *probes,
                          int nprobe, const uint8_t *filter, const uint8_t *exists, int R, int64_t *out_rows,
                          int64_t id_offset, float *out_approx, hipEvent_t *ev, hipStream_t s, bool dense = false,
                          float *out_raw = nullptr, int64_t *pair_stats = nullptr, bool *per_query = nullptr,
                          const ListFp8 *f8 = nullptr) {
    if (per_query) *per_query = false;
    const int64_t E = (int64_t)nq * nprobe;
    IvfParams p{};
    p.plane = plane;
    p.perm = perm;
    p.pnorm = pnorm;
    p.list_off = list_off;
    p.nlist = (int)nlist;
    p.dpad = dpad;
    p.nq = nq;
    p.nprobe = nprobe;
    p.probes = probes;
    p.q_hi = qhi;
    p.qnorm = qnorm;
    p.filter = filter;
    p.exists = exists;
    p.esize = 2;
    if (f8) {
        p.plane8 = f8->plane8;
        p.pscale = f8->pscale;
        p.qexp = f8->qexp;
        p.esize = 1;
    }
    p.lcount = (int *)b.lcount.get(sizeof(int) * nlist);
    p.lfill = (int *)b.lfill.get(sizeof(int) * nlist);
    p.lstart = (int64_t *)b.lstart.get(sizeof(int64_t) * nlist);
    p.lq = (int *)b.lq.get(sizeof(int) * E);
    // 32-query work items when lists are probed by many queries (each A
    // fragment then feeds two MFMAs)
    // (64-query items, QB = 4, measured slower on the dense coarse pass at
    // d = 768: its 99 KiB LDS tile leaves one workgroup per CU)
    // Lists probed by very many queries (IVF-hostile data at large nprobe):
    // 64-query items halve the list re-reads again (10M x 768, nq 1000,
    // nprobe 512 = 51 queries per list: 14.4 -> 12.3 ms; at 13 per list
    // they are slower, tools/index_qg_ab.py).
    p.qg = (!dense && E >= 40 * nlist) ? 64 : (dense || E >= 24 * nlist) ? 32 : 16;
    if (const char *e = tune_env("MQVS_IVF_QG")) {  // A/B knob (tools/ab_split.py style)
        const int v = std::atoi(e);
        if (!dense && (v == 16 || v == 32 || v == 64)) p.qg = v;
    }
    // wide rows: the largest of that size and its smaller siblings whose query
    // tile fits a workgroup's LDS (64 up to dpad 1216, 32 up to 2496, 16 up to
    // 5056 with 160 KiB; the dense plan groups by whatever p.qg is).  The
    // build refuses wider rows, so something fits.
    p.qg = ivf_fit_qg(p.qg, dpad, device_lds_bytes());
    // (p.qg sizes the work items below; the build's own check keeps this from happening)
    if (p.qg == 0) fail(MQVS_ERR_LOGICAL, "list scan: no query tile fits the workgroup's LDS");
    // work items = sum over probed lists of groups x 512-position slices
    // list positions per work item (a multiple of 64): 8 x the item's queries,
    // so the query tile stays a fixed share of the bytes an item reads (round
    // 5: 128 for 16-query items, 512 before -- the item setup's chain of
    // dependent loads was a large part of a 256-position list's scan; mode 3
    // nprobe 1 scan 0.139 -> 0.117 ms, profiles/r05/index_scan/)
    p.chunk = dense ? kIvfChunk : std::max(64, tune_int("MQVS_IVF_CHUNK", 8 * p.qg) / 64 * 64);
    // Pair mode: with about one query per probed list the plan groups
    // nothing; it only orders the pairs (six launches over every list: ~43 us
    // at 39063 lists, nq 1000, nprobe 1).  Instead every (pair, slice) is a
    // work item of its own, each query's region a fixed stride.  Lists probed
    // by several queries are then read once per query (mode 2 at nprobe 1:
    // ~10 % of its list bytes twice).
    const bool pairs = pair_stats && !dense && p.qg == 16 && 16 * E <= nlist && max_list > 0 &&
                       (double)nq * nprobe * (max_list / p.chunk + 1) < 2e9 && tune_int("MQVS_IVF_PAIR", 1) == 1;
    if (pairs) {
        p.pair_stride = (int64_t)nprobe * max_list;
        p.pair_nch = (int)((max_list + p.chunk - 1) / p.chunk);
        p.stats = pair_stats;
        p.cand = (Cand *)b.cand.get(sizeof(Cand) * (size_t)std::max<int64_t>((int64_t)nq * p.pair_stride, 1));
        if (ev) MQVS_HIP(hipEventRecord(ev[2], s));
        launch_ivf_scan(p, metric, tune_int("MQVS_IVF_GRID", 4096), s);
        MQVS_HIP(hipGetLastError());
        if (ev) MQVS_HIP(hipEventRecord(ev[3], s));
        IvfRegions rg;
        rg.stride = p.pair_stride;
        rg.nprobe = nprobe;
        rg.nlist = (int)nlist;
        rg.chunk = p.chunk;
        rg.dpad = dpad;
        rg.esize = p.esize;
        rg.probes = probes;
        rg.list_off = list_off;
        rg.stats = pair_stats;
        const int64_t expect = (int64_t)((double)nprobe * npos / std::max<int64_t>(nlist, 1) * 1.5);
        uint4 *gscr = R > kSortCap ? (uint4 *)b.large.get(sizeof(uint4) * 2 * (size_t)R * nq) : nullptr;
        launch_ivf_select(p.cand, rg, nq, R, metric, out_rows, id_offset, out_approx, expect, s, gscr, out_raw);
        MQVS_HIP(hipGetLastError());
        if (ev) MQVS_HIP(hipEventRecord(ev[4], s));
        if (per_query) *per_query = true;
        return pair_stats;
    }
    const int64_t max_items = (E / p.qg + std::min<int64_t>(E, nlist)) * (max_list / p.chunk + 1);
    p.item_list = (int *)b.items.get(sizeof(int) * max_items);
    p.item_grp = (int *)b.grp.get(sizeof(int) * max_items);
    p.item_chk = (int *)b.chk.get(sizeof(int) * max_items);
    p.nitems = (int *)b.nitems.get(sizeof(int) * 4);
    p.qbase = (int64_t *)b.qbase.get(sizeof(int64_t) * E);
    p.qstart = (int64_t *)b.qstart.get(sizeof(int64_t) * (nq + 1));
    // a query's region is at most min(nprobe * longest list, every position)
    const int64_t cap = (int64_t)nq * std::min<int64_t>((int64_t)nprobe * max_list, npos);
    p.cand = (Cand *)b.cand.get(sizeof(Cand) * (size_t)std::max<int64_t>(cap, 1));
    const int64_t plan_wgs = (nlist + 4095) / 4096;  // k_plan_lists_* workgroups (>= 4096 lists each)
    p.stats = (int64_t *)b.stats.get(sizeof(int64_t) * (8 + 3 * plan_wgs));
    p.bsum = p.stats + 8;
    if (dense)
        launch_ivf_plan_dense(p, npos, s);
    else
        launch_ivf_plan(p, s);
    MQVS_HIP(hipGetLastError());
    if (ev) MQVS_HIP(hipEventRecord(ev[2], s));
    // (a workgroup per work item up to 4096: ~2900 items at nq 1000, nprobe 1)
    launch_ivf_scan(p, metric, dense ? 1024 : tune_int("MQVS_IVF_GRID", 4096), s);
    MQVS_HIP(hipGetLastError());
    if (ev) MQVS_HIP(hipEventRecord(ev[3], s));
    const int64_t expect = dense ? npos : (int64_t)((double)nprobe * npos / std::max<int64_t>(nlist, 1) * 1.5);
    // R above kSortCap: the select sorts through 2 R records of scratch per query
    uint4 *gscr = R > kSortCap ? (uint4 *)b.large.get(sizeof(uint4) * 2 * (size_t)R * nq) : nullptr;
    IvfRegions rg;
    rg.qstart = p.qstart;
    launch_ivf_select(p.cand, rg, nq, R, metric, out_rows, id_offset, out_approx, expect, s, gscr, out_raw);
    MQVS_HIP(hipGetLastError());
    if (ev) MQVS_HIP(hipEventRecord(ev[4], s));
    return p.stats;
}

// mqvs_index_probes sets this for the duration of one search: the coarse
// step's probes[nq][nprobe] are copied there and the search ends
static thread_local int64_t *t_probes_out = nullptr;

// formula_nq: the call's batch size, which selects the exact re-rank's
// distance formula (0: nq; query sub-batches keep the call's, see search.hip)
static void search_index_impl(mqvs_index *ix, const float *queries, int nq, int k, const char *params,
                              const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                              uint32_t flags, hipStream_t user_stream, int formula_nq, int maxv_hint) {
    const int fnq = formula_nq > 0 ? formula_nq : nq;
    check_search_args(ix, "index", ix && ix->binary ? "binary index: search it with mqvs_index_search_binary" : nullptr,
                      nq, k, queries, out_ids, out_dist);
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "nprobe", "num_reorder"}, "search");
    const bool first_stage = flags & MQVS_F_FIRST_STAGE;
    const double alpha = num_param(pm, "alpha", ix->alpha, 1.0, 4.0);
    const int nprobe = pm.count("nprobe")
                           ? (int)num_param(pm, "nprobe", 1, 1, (double)std::min<int64_t>(ix->nlist, kSortCap))
                           : nprobe_of(ix, alpha);
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
                                  out_ids + (size_t)q0 * k, out_dist + (size_t)q0 * k, flags, user_stream, fnq);
            });
            g_istats.nq = nq;
            return;
        }
    }

    mqvs_segment *seg = ix->seg;
    DeviceGuard guard(seg->device);
    IndexWorkspace &ws = index_workspace(seg->device);
    // admission under the workspace budget; every scratch buffer below grows
    // through its gate
    WsScope scope(seg->device, &ws);
    hipStream_t s = user_stream ? user_stream : thread_stream(seg->device);
    scope.set_stream(s);
    // the side stream's variant chain is joined into s on EVERY exit after it
    // forks (an exception between fork and the re-rank's wait included), so
    // the next search on this thread -- whose prep rewrites qvars and status
    // on s -- and a trimmer waiting for s's completion see it finished
    bool forked = false;
    struct JoinGuard {
        hipStream_t s;
        hipEvent_t ev;
        bool &on;
        ~JoinGuard() {
            if (on) (void)hipStreamWaitEvent(s, ev, 0);
        }
    } join_guard{s, ws.join, forked};
    const bool dev = flags & MQVS_F_DEVICE_PTRS;
    const int d = seg->d;
    const bool cos = ix->metric == MQVS_METRIC_COSINE;
    // per-stage timing events only when asked (MQVS_F_TIMING / mqvs_set_timing:
    // ev[0..4]); ev[5] ends every search (the workspace trim waits on it)
    const bool tev = timing_on(flags);
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[0], s));

    const CallIO::In in =
        ws.io.in(queries, sizeof(float) * (size_t)nq * d, filter, exists, (seg->n + 7) / 8, dev, s);
    const float *dq = (const float *)in.queries;
    const uint8_t *dfilter = in.filter, *dexists = in.exists;
    const CallIO::Out out = ws.io.out((size_t)nq * k, dev, out_ids, out_dist);
    int64_t *dids = out.ids;
    float *ddist = out.dist;

    // ---- query prep: cosine re-normalisation variants (the re-rank uses the
    // row's chunk variant, as mqvs_search does), |q|^2.  The variant table
    // starts at kMaxVariants per query with no host round trip; a chain that
    // does not repeat within it on a part of more chunk ordinals (rare:
    // small-integer data) is caught from the status word read at the end, and
    // the search re-runs with the larger table (as mqvs_search does).  The
    // table is not cleared: every variant a reader can select (ordinal < mu +
    // lambda, or < maxv when the chain did not repeat) is written by the prep.
    const int64_t ords = seg->row_offset / seg->granule + (seg->n + seg->granule - 1) / seg->granule;
    const int maxv = cos ? (maxv_hint > 0 ? maxv_hint : kMaxVariants) : 1;
    const int64_t qstride = round_up(d, 32);
    float *qvars = (float *)ws.qvars.get(sizeof(float) * (size_t)nq * maxv * qstride);
    float *qnorms = (float *)ws.qnorms.get(sizeof(float) * nq);
    int *qmu = (int *)ws.qmu.get(sizeof(int) * nq);
    int *qlam = (int *)ws.qlam.get(sizeof(int) * nq);
    // [status 4 ints][pick overflow queries, candidates re-ranked: 2 x u64]
    int *status = (int *)ws.status.get(sizeof(int) * 8);
    launch_fill2(reinterpret_cast<uint32_t *>(status), 8, 0u, nullptr, 0, 0u, s);
    auto *istat = reinterpret_cast<unsigned long long *>(status + 4);
    // the fine pass's per-query stats in pair mode
    auto *pstats = (int64_t *)ws.pstats.get(sizeof(int64_t) * 4 * (size_t)nq);
    bool stats_per_query = false;
    // Cosine: only variant 0 is needed before the exact re-rank (coarse step,
    // list scan), so the rest of the chain -- a sequential fp32 sum per
    // normalisation, up to kMaxVariants of them: 60-130 us at nq 1000 -- runs
    // on the side stream meanwhile and is joined before the re-rank.
    const bool split = cos && !first_stage;
    launch_query_prep(dq, nq, d, cos ? MQVS_METRIC_COSINE : MQVS_METRIC_L2, ix->metric == MQVS_METRIC_L2, qvars, maxv,
                      qnorms, qmu, qlam, status, s, split ? 1 : 0);
    MQVS_HIP(hipGetLastError());
    // The chain starts after the coarse step: beside the coarse batch kernel
    // it slowed that kernel by ~20 us, beside the plan and the list scan it
    // costs less (mode 3, nprobe 1: 0.564 -> 0.544 ms per batch,
    // profiles/r04/index/fork_ab.jsonl).
    float *qdelta = nullptr;  // cosine, pruned re-rank: the chain's variant spread (k_query_prep phase 2)
    auto fork_chain = [&]() {
        MQVS_HIP(hipEventRecord(ws.fork, s));
        MQVS_HIP(hipStreamWaitEvent(ws.side, ws.fork, 0));
        forked = true;
        launch_query_prep(dq, nq, d, MQVS_METRIC_COSINE, false, qvars, maxv, qnorms, qmu, qlam, status, ws.side, 2,
                          qdelta);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipEventRecord(ws.join, ws.side));
    };
    // variant 0 of every query in the list plane's format: bf16, or for an fp8
    // plane the query's own e4m3fn codes (as the bf16 values the scan's MFMA
    // takes) with its scale exponent and norm records (the bf16 rounding is
    // then made only if the coarse step takes the centroid list pass)
    const bool fp8 = ix->plane_fmt == MQVS_INDEX_PLANE_FP8;
    uint16_t *qhi = (uint16_t *)ws.qhi.get(sizeof(uint16_t) * (size_t)nq * ix->dpad);
    uint16_t *q8 = nullptr;
    ListFp8 f8{};
    float *q8rec = nullptr;
    if (fp8) {
        q8 = (uint16_t *)ws.q8.get(sizeof(uint16_t) * (size_t)nq * ix->dpad);
        auto *q8exp = (int16_t *)ws.q8exp.get(sizeof(int16_t) * (size_t)nq);
        q8rec = (float *)ws.q8rec.get(sizeof(float) * kMxRec * (size_t)nq);
        launch_to_fp8(qvars, (int64_t)maxv * qstride, d, nullptr, nq, ix->dpad, nullptr, q8, q8exp, nullptr, nullptr,
                      q8rec, nullptr, s);
        f8 = ListFp8{ix->plane8, ix->pscale, q8exp};
    } else {
        launch_to_bf16(qvars, nq, d, (int64_t)maxv * qstride, qhi, ix->dpad, s);
    }
    MQVS_HIP(hipGetLastError());

    // ---- coarse: the nprobe nearest centroids, by the same list pass over
    // the centroid chunks (every query probes every chunk)
    const int64_t *cprobes = nullptr;  // dense plan: probe r of every query is chunk r
    int64_t *probes = (int64_t *)ws.probes.get(sizeof(int64_t) * (size_t)nq * nprobe);
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
    bool picked = false;
    const int cmode = tune_int("MQVS_IVF_COARSE", 2);
    // (core groups of the pick: nprobe; any count keeps the probes exact,
    // and more of them only score more centroids exactly,
    // profiles/r05/pick/core_t_ab.jsonl)
    float *qrec0 = nullptr;  // variant 0's norm records (the pick's bound; the re-rank pruning's)
    if (nprobe >= ix->nlist) {
        // every list is probed: nothing to rank, and nothing to lose -- the
        // ranked forms never pick a centroid whose score is NaN (a NaN or
        // infinite query; a centroid of a list that holds infinite rows)
        launch_iota_probes(probes, nq, nprobe, s);
        MQVS_HIP(hipGetLastError());
        picked = true;
    }
    if (!picked && cmode == 2 && nprobe <= kCoarsePickMaxT && ix->cent && ix->cent->rows_hi && ix->cent->rows) {
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
        if (launch_scan_p4_groups(cp, ix->coarse_metric, s)) {
            MQVS_HIP(hipGetLastError());
            // each query's bound on |bf16 group value - exact| (the direct
            // formula's rounding terms: the larger of the two)
            float *cbq = (float *)ws.cbq.get(sizeof(float) * (size_t)nq);
            ScanParams bp = cp;
            bp.blas_nq = 1;
            launch_query_bound(bp, ix->coarse_metric, cs->ynorm_max, crec, cs->ynorm_max + 4, cbq, nullptr, s);
            MQVS_HIP(hipGetLastError());
            launch_coarse_pick(cp.p4_gmax, gld, 32 * cp.tiles, nprobe, nprobe, ix->coarse_metric, qvars,
                               (int64_t)maxv * qstride, cs->rows, cs->norms, cs->n, d, cbq, qnorms, 3, nq, probes,
                               istat, s);
            MQVS_HIP(hipGetLastError());
            picked = true;
        }
    }
    if (picked) {
    } else if (tune_int("MQVS_IVF_COARSE", ix->nlist > kCoarseFlatLists ? 1 : 0) == 1) {
        float *pd = (float *)ws.pdist.get(sizeof(float) * (size_t)nq * nprobe);
        search_internal(ix->cent, dq, nq, nprobe, ix->coarse_metric, nullptr, nullptr, probes, pd,
                        MQVS_F_DEVICE_PTRS | (flags & MQVS_F_ASYNC), s);
    } else {
        if (fp8) {
            launch_to_bf16(qvars, nq, d, (int64_t)maxv * qstride, qhi, ix->dpad, s);
            MQVS_HIP(hipGetLastError());
        }
        list_pass(ws.coarse, ix->cplane, ix->cperm, ix->cpnorm, ix->clist_off, ix->cnl, ix->cnpos, ix->cmax,
                  ix->dpad, ix->metric, qhi, qnorms, nq, cprobes, (int)ix->cnl, nullptr, nullptr, nprobe, probes, 0,
                  nullptr, nullptr, s, true);
    }
    if (tev) MQVS_HIP(hipEventRecord(ws.ev[1], s));
    if (t_probes_out) {
        // mqvs_index_probes: the coarse step's lists, nothing after it
        MQVS_HIP(hipMemcpyAsync(t_probes_out, probes, sizeof(int64_t) * (size_t)nq * nprobe, hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipMemcpyAsync(ws.host + 6, istat, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        host_wait(s);
        g_istats.pick_overflow = (int32_t)ws.host[6];
        return;
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
    const bool prune = !first_stage && !(flags & MQVS_F_RERANK_ALL) && ix->yrec && k < R;
    float *craw = nullptr, *ibq = nullptr;
    if (prune) {
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
    if (split) fork_chain();

    // ---- fine: the probed lists
    int64_t *dstats = nullptr;
    if (first_stage) {
        dstats = list_pass(ws.fine, ix->plane, ix->perm, ix->pnorm, ix->list_off, ix->nlist, ix->npos, ix->max_list,
                           ix->dpad, ix->metric, fp8 ? q8 : qhi, qnorms, nq, probes, nprobe, dfilter, dexists, R, dids,
                           seg->row_offset, ddist, tev ? ws.ev : nullptr, s, false, nullptr, pstats,
                           &stats_per_query, fp8 ? &f8 : nullptr);
        MQVS_HIP(hipEventRecord(ws.ev[5], s));
    } else {
        int64_t *crow = (int64_t *)ws.rows.get(sizeof(int64_t) * (size_t)nq * R);
        dstats = list_pass(ws.fine, ix->plane, ix->perm, ix->pnorm, ix->list_off, ix->nlist, ix->npos, ix->max_list,
                           ix->dpad, ix->metric, fp8 ? q8 : qhi, qnorms, nq, probes, nprobe, dfilter, dexists, R, crow, 0,
                           nullptr, tev ? ws.ev : nullptr, s, false, craw, pstats, &stats_per_query,
                           fp8 ? &f8 : nullptr);
        // ---- exact re-rank (needs the whole variant chain)
        if (split) {
            MQVS_HIP(hipStreamWaitEvent(s, ws.join, 0));
            forked = false;
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
        rp.ord_base = (int)(seg->row_offset / seg->granule);
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
        launch_rerank_ids(rp, ix->metric, crow, R, k, seg->row_offset, dids, ddist, rscr, s, pr);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipEventRecord(ws.ev[5], s));
    }

    // decoupled part: results in the new part's row ids (VIWithDataPart.cpp:938-943)
    if (dev && ix->row_ids_map) launch_map_ids(dids, (int64_t)nq * k, ix->row_ids_map, s);
    const bool async = dev && (flags & MQVS_F_ASYNC);
    if (async) {
        const bool variants_matter = !first_stage && ords > maxv;
        launch_async_flags(nullptr, status, variants_matter ? 1 : 0, async_sticky(seg->device, s), s);
        MQVS_HIP(hipGetLastError());
        return;
    }
    int64_t *hs = ws.host;
    int *hst = reinterpret_cast<int *>(ws.host + 4);
    if (!dev) {
        // (host outputs: copied before the final wait)
        if (ix->row_ids_map) launch_map_ids(dids, (int64_t)nq * k, ix->row_ids_map, s);
        ws.io.finish_begin(out, s);
    }
    launch_words_to_host(dstats, 4, status, 8, hs, hst, s, stats_per_query ? dstats : nullptr, nq);
    MQVS_HIP(hipGetLastError());
    host_wait(s);
    if (const int want = first_stage ? 0 : check_variant_chain(*hst, ords, maxv)) {
        search_index_impl(ix, queries, nq, k, params, filter, exists, out_ids, out_dist, flags, user_stream, fnq,
                          want);
        return;
    }
    ws.io.finish_end(out);
    st.values = hs[0];
    st.items = hs[1];
    st.plane_bytes = hs[2];
    st.pairs = hs[3];
    st.pick_overflow = (int32_t)hs[6];  // (istat, copied with the status words)
    st.reranked = hs[7];
    float t[5] = {0, 0, 0, 0, 0}, tot = 0;
    if (tev) {
        for (int i = 0; i < 5; ++i) MQVS_HIP(hipEventElapsedTime(&t[i], ws.ev[i], ws.ev[i + 1]));
        MQVS_HIP(hipEventElapsedTime(&tot, ws.ev[0], ws.ev[5]));
    }
    st.coarse_ms = t[0];
    st.plan_ms = t[1];
    st.scan_ms = t[2];
    st.select_ms = t[3];
    st.rerank_ms = t[4];
    st.total_ms = tot;
    g_istats = st;
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

// ---- persistence: mqvs_index_save / mqvs_index_load -------------------------
// A saved index is the five things a build decides -- centroids, each row's
// list, nlist, alpha, np95 -- behind a 64-byte header, framed as a ClickHouse
// CompressedWriteBuffer stream (include/mqvs.h has the layout byte by byte).
// Everything else is derived again by finish_index.  The framing reuses the
// column ingest's device code in both directions: launch_block_table and
// launch_decode_blocks read it, launch_block_checksum verifies it and, through
// hash_out, computes the checksums the writer stores.

constexpr int64_t kBlobBlock = 1 << 20;  // payload bytes of the blocks mqvs_index_save writes
constexpr int64_t kBlobFrame = 25;       // 16-B checksum + method byte + two UInt32 sizes
constexpr char kBlobMagic[8] = {'M', 'Q', 'V', 'S', 'I', 'D', 'X', '\0'};
constexpr int kFingerprintRows = 1024;

struct BlobHeader {  // little-endian, as the host is
    char magic[8];
    uint32_t version, kind, metric, dim;
    uint64_t n, nlist;
    uint32_t alpha_bits, np95;
    uint64_t fingerprint;
    uint32_t plane_fmt;  // MQVS_INDEX_PLANE_* (zero on a binary index)
    uint8_t reserved[4];
};
static_assert(sizeof(BlobHeader) == MQVS_INDEX_BLOB_HEADER_BYTES, "the documented header");

static void put_block_header(uint8_t *h, uint32_t payload) {  // h: the 9 bytes after the checksum
    const uint32_t csize = payload + 9;
    h[0] = 0x02;
    for (int i = 0; i < 4; ++i) {
        h[1 + i] = (uint8_t)(csize >> (8 * i));
        h[5 + i] = (uint8_t)(payload >> (8 * i));
    }
}

static int64_t row_bytes_of(const mqvs_segment *seg) { return seg->binary ? seg->code_bytes : 4 * (int64_t)seg->d; }

// The fingerprint of a segment's resident rows: S = min(n, 1024) rows, row
// floor(i n / S) for i < S (the builds' sample rule), gathered back to back (a
// float row as its d fp32 values as they are resident -- normalised for a
// cosine segment --, a binary row as its dim_bits / 8 code bytes) and framed as
// the payload of one method-NONE block; the fingerprint is the low 64 bits of
// that block's CityHash128 checksum (k_block_checksum, one lane).  The rows are
// read through seg->rows / seg->codes, which for rows moved to host memory is
// the mapped address of the pinned copy.
static uint64_t segment_fingerprint(mqvs_segment *seg, hipStream_t s) {
    const int64_t n = seg->n, S = std::min<int64_t>(n, kFingerprintRows), rb = row_bytes_of(seg);
    const int64_t len = S * rb;
    // the block starts at byte 7, so that its payload starts at byte 32
    TmpBuf buf(32 + (size_t)len + 16), tab(sizeof(IngestBlock)), out(sizeof(uint64_t) * 2 + sizeof(int) * 2);
    uint8_t pre[32] = {};
    put_block_header(pre + 23, (uint32_t)len);
    IngestBlock b{};
    b.src = 32;
    b.csize = b.usize = (uint32_t)len;
    b.method = 0x02;
    MQVS_HIP(hipMemcpyAsync(buf.p, pre, 32, hipMemcpyHostToDevice, s));
    MQVS_HIP(hipMemcpyAsync(tab.p, &b, sizeof(b), hipMemcpyHostToDevice, s));
    MQVS_HIP(hipMemsetAsync(out.p, 0, sizeof(uint64_t) * 2 + sizeof(int) * 2, s));
    std::vector<int64_t> idx64(S);
    std::vector<int32_t> idx32(S);
    for (int64_t i = 0; i < S; ++i) idx32[i] = (int32_t)(idx64[i] = (int64_t)((__int128)i * n / S));
    TmpBuf didx(sizeof(int64_t) * std::max<int64_t>(S, 1)), wide(seg->binary ? sizeof(uint32_t) * (size_t)S * seg->code_words : 0);
    if (S > 0 && seg->binary) {
        MQVS_HIP(hipMemcpyAsync(didx.p, idx32.data(), sizeof(int32_t) * S, hipMemcpyHostToDevice, s));
        launch_bivf_gather(seg->codes, seg->code_words, didx.as<int32_t>(), S, wide.as<uint32_t>(), s);
        MQVS_HIP(hipMemcpy2DAsync(buf.as<uint8_t>() + 32, (size_t)rb, wide.p, (size_t)seg->code_words * 4, (size_t)rb,
                                  (size_t)S, hipMemcpyDeviceToDevice, s));
    } else if (S > 0) {
        MQVS_HIP(hipMemcpyAsync(didx.p, idx64.data(), sizeof(int64_t) * S, hipMemcpyHostToDevice, s));
        launch_gather_rows(seg->rows, seg->d, seg->d, didx.as<int64_t>(), S, (float *)(buf.as<uint8_t>() + 32), s);
    }
    uint64_t *hash = out.as<uint64_t>();
    launch_block_checksum(buf.as<uint8_t>(), tab.as<IngestBlock>(), 1, 1, (int *)(hash + 2), hash, s);
    MQVS_HIP(hipGetLastError());
    uint64_t h[2] = {};
    MQVS_HIP(hipMemcpyAsync(h, hash, sizeof(h), hipMemcpyDeviceToHost, s));
    MQVS_HIP(hipStreamSynchronize(s));
    return h[0];
}

static int64_t blob_content_bytes(const mqvs_index *ix) {
    return (int64_t)sizeof(BlobHeader) + ix->nlist * row_bytes_of(ix->seg) + 4 * ix->seg->n;
}

static size_t blob_bytes(const mqvs_index *ix) {
    const int64_t content = blob_content_bytes(ix);
    return (size_t)(content + kBlobFrame * ((content + kBlobBlock - 1) / kBlobBlock));
}

static size_t save_impl(mqvs_index *ix, uint8_t *out, size_t cap) {
    if (!ix || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
    mqvs_segment *seg = ix->seg;
    const int64_t n = seg->n, L = ix->nlist, rb = row_bytes_of(seg), cb = L * rb;
    const int64_t content = blob_content_bytes(ix), nb = (content + kBlobBlock - 1) / kBlobBlock;
    const size_t total = blob_bytes(ix);
    if (cap < total)
        fail(MQVS_ERR_BAD_ARGUMENTS, "output holds " + std::to_string(cap) + " bytes, " + std::to_string(total) + " needed");
    DeviceGuard guard(seg->device);
    hipStream_t s = thread_stream(seg->device);
    BlobHeader hd{};
    std::memcpy(hd.magic, kBlobMagic, 8);
    hd.version = MQVS_INDEX_BLOB_VERSION;
    hd.kind = ix->binary ? MQVS_INDEX_KIND_BINARY_IVF : MQVS_INDEX_KIND_FLOAT_IVF;
    hd.metric = (uint32_t)ix->metric;
    hd.dim = (uint32_t)seg->d;
    hd.n = (uint64_t)n;
    hd.nlist = (uint64_t)L;
    std::memcpy(&hd.alpha_bits, &ix->alpha, 4);
    hd.np95 = (uint32_t)ix->np95;
    hd.fingerprint = segment_fingerprint(seg, s);
    hd.plane_fmt = ix->binary ? 0u : (uint32_t)ix->plane_fmt;

    // ---- the content: header, centroid table, canonical assignment
    TmpBuf cont((size_t)content), asg(sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1));
    uint8_t *c = cont.as<uint8_t>();
    MQVS_HIP(hipMemcpyAsync(c, &hd, sizeof(hd), hipMemcpyHostToDevice, s));
    if (ix->binary)
        MQVS_HIP(hipMemcpy2DAsync(c + sizeof(hd), (size_t)rb, ix->bcent, (size_t)seg->code_words * 4, (size_t)rb,
                                  (size_t)L, hipMemcpyDeviceToDevice, s));
    else
        MQVS_HIP(hipMemcpyAsync(c + sizeof(hd), ix->cent->rows, (size_t)cb, hipMemcpyDeviceToDevice, s));
    if (n > 0) {
        // the list of a position, scattered to its row; rows at no position: -1
        MQVS_HIP(hipMemsetAsync(asg.p, 0xFF, sizeof(int32_t) * (size_t)n, s));
        launch_grp_assign_of(ix->perm, ix->list_off, L, ix->npos, n, asg.as<int32_t>(), s);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(c + sizeof(hd) + cb, asg.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
    }
    // ---- the frame: method NONE blocks of at most kBlobBlock bytes
    TmpBuf framed(total), tab(sizeof(IngestBlock) * (size_t)nb), hashes(16 * (size_t)nb + 16);
    std::vector<uint8_t> heads((size_t)nb * kBlobFrame, 0);
    std::vector<IngestBlock> ht((size_t)nb);
    for (int64_t i = 0; i < nb; ++i) {
        const uint32_t len = (uint32_t)std::min(kBlobBlock, content - i * kBlobBlock);
        put_block_header(heads.data() + i * kBlobFrame + 16, len);
        ht[i].src = i * (kBlobBlock + kBlobFrame) + kBlobFrame;
        ht[i].dst = i * kBlobBlock;
        ht[i].csize = ht[i].usize = len;
        ht[i].method = 0x02;
        ht[i].pad = 0;
    }
    uint8_t *f = framed.as<uint8_t>();
    const size_t pitch = (size_t)(kBlobBlock + kBlobFrame);
    MQVS_HIP(hipMemcpy2DAsync(f, pitch, heads.data(), (size_t)kBlobFrame, (size_t)kBlobFrame, (size_t)nb,
                              hipMemcpyHostToDevice, s));
    const int64_t full = content / kBlobBlock, rest = content - full * kBlobBlock;
    if (full > 0)
        MQVS_HIP(hipMemcpy2DAsync(f + kBlobFrame, pitch, c, (size_t)kBlobBlock, (size_t)kBlobBlock, (size_t)full,
                                  hipMemcpyDeviceToDevice, s));
    if (rest > 0)
        MQVS_HIP(hipMemcpyAsync(f + full * pitch + kBlobFrame, c + full * kBlobBlock, (size_t)rest,
                                hipMemcpyDeviceToDevice, s));
    MQVS_HIP(hipMemcpyAsync(tab.p, ht.data(), sizeof(IngestBlock) * (size_t)nb, hipMemcpyHostToDevice, s));
    uint64_t *hash = hashes.as<uint64_t>();
    // (the verdict word of the checksum pass is not read: the stored checksums are still zero)
    launch_block_checksum(f, tab.as<IngestBlock>(), nb, 1, (int *)(hash + 2 * nb), hash, s);
    MQVS_HIP(hipGetLastError());
    MQVS_HIP(hipMemcpy2DAsync(f, pitch, hash, 16, 16, (size_t)nb, hipMemcpyDeviceToDevice, s));
    MQVS_HIP(hipMemcpyAsync(out, f, total, hipMemcpyDeviceToHost, s));
    MQVS_HIP(hipStreamSynchronize(s));
    return total;
}

// the header of a decoded blob; throws what the error table of include/mqvs.h names
static void check_blob_header(const BlobHeader &hd) {
    if (std::memcmp(hd.magic, kBlobMagic, 8) != 0) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: bad magic");
    if (hd.version != MQVS_INDEX_BLOB_VERSION)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "index blob: format version " + std::to_string(hd.version) + " is not implemented");
    float alpha;
    std::memcpy(&alpha, &hd.alpha_bits, 4);
    const bool fl = hd.kind == MQVS_INDEX_KIND_FLOAT_IVF, bi = hd.kind == MQVS_INDEX_KIND_BINARY_IVF;
    const bool metric_ok = fl ? (hd.metric == MQVS_METRIC_L2 || hd.metric == MQVS_METRIC_IP || hd.metric == MQVS_METRIC_COSINE)
                              : (hd.metric == MQVS_METRIC_HAMMING || hd.metric == MQVS_METRIC_JACCARD);
    if ((!fl && !bi) || !metric_ok || hd.nlist < 1 || hd.nlist > (1u << 20) || hd.n >= ((uint64_t)1 << 31) ||
        (hd.n > 0 && hd.nlist > hd.n) || !(alpha >= 1.0f && alpha <= 4.0f) || hd.np95 > (uint32_t)kSortCap ||
        hd.dim == 0 || hd.dim > (1u << 24) || (bi && hd.dim % 8) ||
        (hd.plane_fmt != MQVS_INDEX_PLANE_BF16 && (bi || hd.plane_fmt != MQVS_INDEX_PLANE_FP8)))
        fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: malformed header");
}

static mqvs_index *load_impl(mqvs_segment *seg, const uint8_t *blob, size_t bytes) {
    if (!seg || !blob) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
    if (bytes < (size_t)kBlobFrame + sizeof(BlobHeader)) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: truncated");
    const int64_t n = seg->n, rb = row_bytes_of(seg);
    DeviceGuard guard(seg->device);
    hipStream_t s = thread_stream(seg->device);
    hipEvent_t e0, e1;
    MQVS_HIP(hipEventCreate(&e0));
    MQVS_HIP(hipEventCreate(&e1));
    mqvs_index *ix = nullptr;
    try {
        MQVS_HIP(hipEventRecord(e0, s));
        // ---- the block chain, its checksums, the decoded content
        const int64_t maxb = (int64_t)bytes / kBlobFrame + 1;
        TmpBuf dblob(bytes), tab(sizeof(IngestBlock) * (size_t)maxb), words(sizeof(int64_t) * 4);
        MQVS_HIP(hipMemcpyAsync(dblob.p, blob, bytes, hipMemcpyHostToDevice, s));
        launch_block_table(dblob.as<uint8_t>(), (int64_t)bytes, tab.as<IngestBlock>(), maxb, words.as<int64_t>(), s);
        MQVS_HIP(hipGetLastError());
        int64_t tb[3] = {};
        MQVS_HIP(hipMemcpyAsync(tb, words.p, sizeof(tb), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipStreamSynchronize(s));
        // (no codec expands more than 256-fold: a larger claim is not allocated)
        if (tb[2] || tb[1] < (int64_t)sizeof(BlobHeader) || tb[1] / 256 > (int64_t)bytes)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: truncated or malformed compressed block chain");
        const int64_t nblk = tb[0], total = tb[1];
        constexpr int kBadChecksum = 8;  // (the decode raises 4)
        int *status = (int *)(words.as<int64_t>() + 3);
        MQVS_HIP(hipMemsetAsync(status, 0, sizeof(int), s));
        TmpBuf cont((size_t)total);
        uint8_t *c = cont.as<uint8_t>();
        launch_block_checksum(dblob.as<uint8_t>(), tab.as<IngestBlock>(), nblk, kBadChecksum, status, nullptr, s);
        launch_decode_blocks(dblob.as<uint8_t>(), (int64_t)bytes, tab.as<IngestBlock>(), nblk, c, status, s);
        MQVS_HIP(hipGetLastError());
        int hstatus = 0;
        BlobHeader hd{};
        MQVS_HIP(hipMemcpyAsync(&hstatus, status, sizeof(int), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipMemcpyAsync(&hd, c, sizeof(hd), hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipStreamSynchronize(s));
        if (hstatus & kBadChecksum)
            fail(MQVS_ERR_CHECKSUM, "Checksum doesn't match: corrupted data (index blob, CityHash128 of a compressed block)");
        if (hstatus) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: malformed LZ4 block (CANNOT_DECOMPRESS)");
        // ---- the header against itself, then against the segment
        check_blob_header(hd);
        const bool binary = hd.kind == MQVS_INDEX_KIND_BINARY_IVF;
        const int64_t L = (int64_t)hd.nlist;
        const int64_t hrb = binary ? hd.dim / 8 : 4 * (int64_t)hd.dim, cb = L * hrb;
        if (total != (int64_t)sizeof(BlobHeader) + cb + 4 * (int64_t)hd.n)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: " + std::to_string(total) + " bytes of content, the header implies " +
                                              std::to_string((int64_t)sizeof(BlobHeader) + cb + 4 * (int64_t)hd.n));
        if (binary != seg->binary)
            fail(MQVS_ERR_LOGICAL, std::string("index blob: a ") + (binary ? "binary" : "Float32") + " index on a " +
                                       (seg->binary ? "binary" : "Float32") + " segment");
        if ((int64_t)hd.n != n || (int64_t)hd.dim != seg->d)
            fail(MQVS_ERR_LOGICAL, "index blob: saved over " + std::to_string(hd.n) + " rows of dimension " +
                                       std::to_string(hd.dim) + ", the segment has " + std::to_string(n) + " of " +
                                       std::to_string(seg->d));
        if (!binary && ((int)hd.metric == MQVS_METRIC_COSINE) != (seg->metric == MQVS_METRIC_COSINE))
            fail(MQVS_ERR_LOGICAL, "segment was prepared for a different metric (cosine segments are normalised in HBM)");
        if (!binary) check_index_width(seg);
        if (hd.fingerprint != segment_fingerprint(seg, s))
            fail(MQVS_ERR_LOGICAL, "index blob: saved over other rows than the segment's (fingerprint mismatch)");

        // ---- the index
        ix = new mqvs_index();
        ix->seg = seg;
        ix->binary = binary;
        ix->metric = (int)hd.metric;
        ix->nlist = L;
        std::memcpy(&ix->alpha, &hd.alpha_bits, 4);
        ix->np95 = (int)hd.np95;
        if (binary) {
            ix->coarse_metric = MQVS_METRIC_HAMMING;
            const size_t cwb = (size_t)seg->code_words * 4;
            ix->bcent = dalloc<uint32_t>(ix, (size_t)L * seg->code_words);
            MQVS_HIP(hipMemsetAsync(ix->bcent, 0, cwb * (size_t)L, s));
            MQVS_HIP(hipMemcpy2DAsync(ix->bcent, cwb, c + sizeof(hd), (size_t)rb, (size_t)rb, (size_t)L,
                                      hipMemcpyDeviceToDevice, s));
        } else {
            ix->coarse_metric = ix->metric == MQVS_METRIC_L2 ? MQVS_METRIC_L2 : kMetricIpRaw;
            ix->dpad = round_up(seg->d, kBfK);
            ix->plane_fmt = (int)hd.plane_fmt;
            ix->cent = segment_from_device((const float *)(c + sizeof(hd)), L, seg->d,
                                           ix->metric == MQVS_METRIC_L2 ? MQVS_METRIC_L2 : MQVS_METRIC_IP, s);
        }
        // (the assignment follows a binary centroid table at any byte offset)
        TmpBuf asg(sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1));
        if (n > 0)
            MQVS_HIP(hipMemcpyAsync(asg.p, c + sizeof(hd) + cb, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
        finish_index(ix, asg.as<int32_t>(), true, s);
        MQVS_HIP(hipEventRecord(e1, s));
        MQVS_HIP(hipStreamSynchronize(s));
        float ms = 0.f;
        MQVS_HIP(hipEventElapsedTime(&ms, e0, e1));
        ix->build_ms = ms;
        if (ix->cent) ix->bytes += ix->cent->bytes;
    } catch (...) {
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (ix) free_index(ix);
        throw;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ix;
}

// host only: the header of a blob whose first block is stored (method NONE)
static void blob_info_impl(const uint8_t *blob, size_t bytes, mqvs_index_blob_info_t *out) {
    if (!blob || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
    if (bytes < (size_t)kBlobFrame + sizeof(BlobHeader)) fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: truncated");
    const uint8_t *h = blob + 16;
    auto u32 = [](const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); };
    if (h[0] == 0x82) fail(MQVS_ERR_NOT_IMPLEMENTED, "index blob: the first block is LZ4-compressed (load it, or decompress it first)");
    const uint32_t csize = u32(h + 1), usize = u32(h + 5);
    if (h[0] != 0x02 || csize < 9 || csize - 9 != usize || usize < sizeof(BlobHeader) || 16 + (size_t)csize > bytes)
        fail(MQVS_ERR_ILLEGAL_COLUMN, "index blob: malformed first block");
    BlobHeader hd;
    std::memcpy(&hd, blob + kBlobFrame, sizeof(hd));
    check_blob_header(hd);
    std::memset(out, 0, sizeof(*out));
    out->version = hd.version;
    out->kind = hd.kind;
    out->metric = (int32_t)hd.metric;
    out->dim = (int32_t)hd.dim;
    out->n = (int64_t)hd.n;
    out->nlist = (int64_t)hd.nlist;
    std::memcpy(&out->alpha, &hd.alpha_bits, 4);
    out->np95 = (int32_t)hd.np95;
    out->fingerprint = hd.fingerprint;
    const int64_t hrb = hd.kind == MQVS_INDEX_KIND_BINARY_IVF ? hd.dim / 8 : 4 * (int64_t)hd.dim;
    out->content_bytes = (uint64_t)((int64_t)sizeof(BlobHeader) + (int64_t)hd.nlist * hrb + 4 * (int64_t)hd.n);
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

int mqvs_index_search(mqvs_index_t idx, const float *queries, int32_t nq, int32_t k, const char *params,
                      const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                      uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{4, (uint64_t)(uintptr_t)idx, (uint64_t)nq, (uint64_t)k, wait_str_hash(params), filter != nullptr,
                      row_exists != nullptr, flags};
        search_index_impl(idx, queries, nq, k, params, filter, row_exists, out_ids, out_dist, flags,
                          (hipStream_t)stream, 0);
    });
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
