// index_internal.h -- what the index path's files share: index.hip (the
// thread's workspace, the parameter parser, C glue), index_build.hip (the
// builds), index_search.hip and index_search_binary.hip (the float and the
// binary index search) and index_blob.hip (save / load).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "index_kernels.h"
#include "search_host.h"

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
// through the thread's FLAT workspace gate (the WsScope of SearchAdmission), so
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
    // an ASYNC search with a flag word of the caller's left its stats in
    // `host`: index_collect_stats reads them after the caller's sync
    bool pending = false, pending_tev = false;
    mqvs_index_search_stats pending_st{};
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

// ---- index.hip
extern thread_local mqvs_index_search_stats g_istats;  // mqvs_index_last_stats
IndexWorkspace &index_workspace(int device);
// Search::Parameters: "k=v,k=v"
std::map<std::string, std::string> parse_params(const char *s);
double num_param(const std::map<std::string, std::string> &m, const std::string &key, double dflt, double lo,
                 double hi);
void check_keys(const std::map<std::string, std::string> &m, const std::vector<std::string> &valid, const char *what);
int nprobe_of(const mqvs_index *ix, double alpha);
void free_index(mqvs_index *ix);

// ---- index_build.hip
mqvs_index *build_impl(mqvs_segment *seg, const char *index_type, const char *params);
// a binary metric by name (`what`: the parameter, for the message)
int binary_metric_of(const std::string &name, const char *what);
void check_index_width(mqvs_segment *seg);
void finish_index(mqvs_index *ix, const int32_t *assign, bool from_blob, hipStream_t s);

// ---- index_search.hip
// The admission of one search to the thread's workspace on the segment's
// device: the workspace's budget gate (every scratch buffer of the stages
// grows through it) is held, and the search's stream named to it, for the
// scope's life.
struct SearchAdmission {
    DeviceGuard guard;
    IndexWorkspace &ws;
    WsScope scope;
    const hipStream_t s;
    SearchAdmission(mqvs_segment *seg, hipStream_t user_stream)
        : guard(seg->device), ws(index_workspace(seg->device)), scope(seg->device, &ws),
          s(user_stream ? user_stream : thread_stream(seg->device)) {
        scope.set_stream(s);
    }
};
int search_nprobe(const mqvs_index *ix, const std::map<std::string, std::string> &pm);
void index_read_stats(IndexWorkspace &ws, mqvs_index_search_stats st, bool tev, bool binary);
void search_index_impl(mqvs_index *ix, const float *queries, int nq, int k, const char *params, const uint8_t *filter,
                       const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags,
                       hipStream_t user_stream, int formula_nq, int maxv_hint = 0, int64_t ord_base = -1,
                       int *async_word = nullptr, int64_t *probes_out = nullptr);
// the stats of this thread's last ASYNC search with a flag word of the
// caller's (sharded.hip's fast path), after the caller's stream sync
void index_collect_stats(int device);

// ---- index_search_binary.hip
void search_binary_index_impl(mqvs_index *ix, const uint8_t *queries, int nq, int k, const char *params,
                              const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                              uint32_t flags, hipStream_t user_stream, int64_t *probes_out);
// with the search parameters resolved (metric Hamming or Jaccard, 1 <= nprobe <= nlist)
void search_binary_index_impl(mqvs_index *ix, const uint8_t *queries, int nq, int k, int metric, int nprobe,
                              const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                              uint32_t flags, hipStream_t user_stream, int64_t *probes_out);
// a query's record region of a binary index search: at most every position of its probed lists
inline int64_t binary_index_cap(const mqvs_index *ix, int nprobe) {
    return std::max<int64_t>(1, std::min<int64_t>((int64_t)nprobe * ix->max_list, ix->npos));
}
// a query's scratch bytes of one: its records, and its centroid distances when the lists are ranked
inline int64_t binary_index_scratch(const mqvs_index *ix, int nprobe) {
    return binary_index_cap(ix, nprobe) * (int64_t)sizeof(Cand) + (nprobe < ix->nlist ? ix->nlist * 4 : 0);
}

// ---- index_blob.hip
size_t blob_bytes(const mqvs_index *ix);
size_t save_impl(mqvs_index *ix, uint8_t *out, size_t cap);
mqvs_index *load_impl(mqvs_segment *seg, const uint8_t *blob, size_t bytes);
void blob_info_impl(const uint8_t *blob, size_t bytes, mqvs_index_blob_info_t *out);

}  // namespace mqvs
