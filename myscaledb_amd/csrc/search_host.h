// search_host.h -- the host side the search entry points share: the staging
// of a call's inputs and outputs (CallIO), the argument rules every entry
// point applies the same way, and the searches the host files call in one
// another.  Included by workspace.h and index_internal.h (and cache.hip); no
// kernel file sees it.
#pragma once

#include "mqvs_internal.h"

namespace mqvs {

// The inputs and outputs of one search call on the device.  A call with
// MQVS_F_DEVICE_PTRS (`dev`) uses the caller's pointers as they are; a
// host-pointer call is staged through the pinned buffers (HostBuf) into
// gated device buffers, and its results come back the same way.  Workspace
// and IndexWorkspace hold one each: an index search's nested FLAT searches
// must not reuse the outer call's buffers.
struct CallIO {
    GBuf queries, filter, exists, out_ids, out_dist;
    struct In {
        const void *queries;
        const uint8_t *filter, *exists;
    };
    // queries (`bytes`; none staged when null) and the two row bitmaps
    // (bm_bytes each, either may be null): the CPU copies now, the DMAs on s
    In in(const void *q, size_t bytes, const uint8_t *flt, const uint8_t *ex, size_t bm_bytes, bool dev,
          hipStream_t s) {
        if (dev) return In{q, flt, ex};
        In r{nullptr, nullptr, nullptr};
        if (q) r.queries = put(queries, pin_q, q, bytes, s);
        if (flt) r.filter = (const uint8_t *)put(filter, pin_f, flt, bm_bytes, s);
        if (ex) r.exists = (const uint8_t *)put(exists, pin_e, ex, bm_bytes, s);
        return r;
    }
    // a host array other than a bitmap (mqvs_rerank's candidate rows) through
    // the filter bitmap's slot
    const void *in_list(const void *src, size_t bytes, hipStream_t s) { return put(filter, pin_f, src, bytes, s); }
    // m ids and distances: where the kernels write them, and where they go
    struct Out {
        int64_t *ids;
        float *dist;
        int64_t *host_ids;  // null: the caller's device arrays, nothing to copy back
        float *host_dist;
        size_t m;
    };
    Out out(size_t m, bool dev, int64_t *ids, float *dist) {
        if (dev) return Out{ids, dist, nullptr, nullptr, m};
        return Out{(int64_t *)out_ids.get(sizeof(int64_t) * m), (float *)out_dist.get(sizeof(float) * m), ids, dist,
                   m};
    }
    // the results of a host-pointer call in two halves, so the call's last
    // host_wait covers the copies: begin queues device -> pinned on s, end
    // (after that wait) copies pinned -> the caller's arrays
    void finish_begin(const Out &o, hipStream_t s) {
        if (!o.host_ids) return;
        auto *h = (unsigned char *)pin_o.get(12 * o.m);
        if (!o.m) return;
        MQVS_HIP(hipMemcpyAsync(h, o.ids, 8 * o.m, hipMemcpyDeviceToHost, s));
        MQVS_HIP(hipMemcpyAsync(h + 8 * o.m, o.dist, 4 * o.m, hipMemcpyDeviceToHost, s));
    }
    void finish_end(const Out &o) {
        if (!o.host_ids || !o.m) return;
        const auto *h = (const unsigned char *)pin_o.p;
        std::memcpy(o.host_ids, h, 8 * o.m);
        std::memcpy(o.host_dist, h + 8 * o.m, 4 * o.m);
    }
    // both halves around a host_wait of their own
    void finish(const Out &o, hipStream_t s) {
        if (!o.host_ids) return;
        finish_begin(o, s);
        host_wait(s);
        finish_end(o);
    }
    // the device buffers' bytes, freed (the pinned ones too: host memory, not counted)
    size_t release() {
        size_t b = 0;
        for (GBuf *x : {&queries, &filter, &exists, &out_ids, &out_dist}) {
            b += x->cap;
            x->release();
        }
        for (HostBuf *x : {&pin_q, &pin_f, &pin_e, &pin_o}) x->release();
        return b;
    }

   private:
    HostBuf pin_q, pin_f, pin_e, pin_o;
    // host -> device through `pin`
    static void *put(GBuf &dst, HostBuf &pin, const void *src, size_t bytes, hipStream_t s) {
        void *d = dst.get(bytes);
        if (bytes) {
            void *h = pin.get(bytes);
            std::memcpy(h, src, bytes);
            MQVS_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
        }
        return d;
    }
};

// ---------------------------------------------------------------------------
// What every search entry point does the same way (search.hip,
// search_binary.hip, index.hip)

// `what`: "segment" or "index"; wrong_kind: null, or what to say when the
// handle is of the other kind (float / binary) than the entry point serves
inline void check_search_args(const void *handle, const char *what, const char *wrong_kind, int nq, int k,
                              const void *queries, const void *out_ids, const void *out_dist) {
    if (!handle) fail(MQVS_ERR_BAD_ARGUMENTS, std::string("null ") + what);
    if (wrong_kind) fail(MQVS_ERR_LOGICAL, wrong_kind);
    if (nq < 0 || k < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "nq and k must be non-negative");
    if (nq > 0 && k > 0 && (!queries || !out_ids || !out_dist))
        fail(MQVS_ERR_BAD_ARGUMENTS, "null query or output pointer");
    if (k > kMaxK) fail(MQVS_ERR_BAD_ARGUMENTS, "k above " + std::to_string(kMaxK) + " not supported");
}

// fn(q0, m) for the query sub-batches [q0, q0 + m) of at most qb queries
// (queries are independent searches: the entry points re-invoke themselves)
template <typename F>
inline void for_query_batches(int nq, int64_t qb, F &&fn) {
    for (int64_t q0 = 0; q0 < nq; q0 += qb) fn((int)q0, (int)std::min<int64_t>(qb, nq - q0));
}

// A cosine query whose re-normalisation does not repeat within maxv steps
// (`status` set by the query prep) is exact only on the part's first maxv
// chunk ordinals.  Returns the larger table size to re-run the search with,
// 0 when nothing is wrong (maxv covers every ordinal unless the part has more
// than kMaxVariantsCap chunks); fails when the largest table did not do, or
// when the caller cannot re-run (can_retry false).
inline int check_variant_chain(int status, int64_t ords, int maxv, bool can_retry = true) {
    if (!status || ords <= maxv) return 0;
    const int want = (int)std::min<int64_t>(ords, kMaxVariantsCap);
    if (can_retry && maxv < want) return want;
    fail(MQVS_ERR_LOGICAL, "cosine query normalisation did not repeat within " + std::to_string(maxv) +
                               " steps on a part of more chunks");
}

// Large k (above the LDS sort): the global-scratch sort of the final select,
// and query sub-batches small enough that the candidate lists and the dense
// probe matrix stay within a fixed HBM budget.
inline int large_k_cap(int k) { return (int)std::min<int64_t>(kCandMax, (int64_t)16 * k); }
inline int large_k_batch(int64_t n, int k) {
    const int64_t cap = large_k_cap(k);
    const int64_t probe = std::min<int64_t>(n, (int64_t)((double)k * (double)n / (double)(cap / 3)) + 1);
    const int64_t budget = (int64_t)scratch_budget();
    const int64_t by_cand = budget / 8 / cap;                          // 8-B candidates
    const int64_t by_probe = budget / 4 / std::max<int64_t>(probe, 1);  // fp32 probe values
    return (int)std::max<int64_t>(1, std::min(by_cand, by_probe));
}
// candidate capacity per query (a fixed budget spread over the batch)
inline int cand_capacity(int nq, int k) {
    const int cap = (int)std::min<int64_t>(kCandMax, kCandBudget / std::max(nq, 1));
    return std::max(cap, k > kSortCap ? large_k_cap(k) : kSortCap) / 256 * 256;
}

// What mqvs.hip keeps per thread and per process: the stats of the thread's last search
// (mqvs_last_search_stats), and the per-call mode flags resolved against the
// process-wide defaults (mqvs_set_*)
mqvs_search_stats &search_stats();
int call_batch_mode(uint32_t flags);   // 0: bf16 pre-filter + exact re-rank when possible, 1: fp32 MFMA
int call_gather_mode(uint32_t flags);  // selective PREWHERE: 0 never gather, 1 when <= 60% selected, 2 always

// ---------------------------------------------------------------------------
// The searches behind the C ABI, as the host files call them

// FLAT search of a segment (MergeTreeVSManager::vectorScanWithoutIndex);
// metric may be kMetricIpRaw (faiss knn_inner_product contract)
void search_internal(mqvs_segment *seg, const float *queries, int nq, int k, int metric,
                     const uint8_t *filter, const uint8_t *exists, int64_t *out_ids, float *out_dist,
                     uint32_t flags, hipStream_t stream, int64_t ord_base = -1);
// mqvs_search with device pointers on `stream` (sharded.hip)
void search_segment(mqvs_segment *seg, const float *queries, int nq, int k, int metric, const uint8_t *filter,
                    const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t stream,
                    int64_t ord_base);
// the same, asynchronous: no host sync; the fallback flags (bit 0 candidate
// overflow, bit 1 cosine variant table too short) are OR-ed into *flag_word,
// and search_collect_stats(device) fills the thread's stats after the
// caller's stream sync
void search_segment_async(mqvs_segment *seg, const float *queries, int nq, int k, int metric, const uint8_t *filter,
                          const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags,
                          hipStream_t stream, int64_t ord_base, int *flag_word);
void search_collect_stats(int device);
// the other searches behind the C ABI (search.hip, search_binary.hip)
void rerank_flat(mqvs_segment *seg, const float *queries, int nq, const int64_t *cand, int ncand, int k, int metric,
                 const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t stream);
void search_binary(mqvs_segment *seg, const uint8_t *queries, int nq, int k, int metric, const uint8_t *filter,
                   const uint8_t *exists, int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t stream);
// segment.hip's services for the other paths:
// rows of `nbytes` (host or device) -> zero-padded [n][words] on the device
void upload_codes(uint32_t *dst, int words, const uint8_t *src, int64_t nbytes, int64_t n, bool dev, hipStream_t s);
// segment from rows already on the current device (copied); granule = n
mqvs_segment *segment_from_device(const float *dev_rows, int64_t n, int d, int metric, hipStream_t st);
void segment_release(mqvs_segment *s);
// the calling thread's ASYNC sticky word on `device` (launch_async_flags ORs
// a search's flags into it; mqvs_async_check reads and clears it)
int *async_sticky(int device, hipStream_t s);
// the segment an index was built over (cache.hip validates put pairs)
mqvs_segment *index_segment(mqvs_index *idx);
void index_thread_release();  // index.hip: the calling thread's index workspaces

}  // namespace mqvs
