// mqvs.hip -- what the C ABI of libmqvs.so keeps per thread and per process,
// and the entry points that are not a segment's, a workspace's or an index's:
//   * the thread's last error and search stats, and the process-wide mode
//     flags (batch, gather, timing, scratch budget) with their setters;
//   * the fault drill (mqvs_inject_fault);
//   * the cached device attributes the launchers size their grids by;
//   * mqvs_init, mqvs_device_count, mqvs_thread_release, mqvs_shutdown;
//   * the search entry points, which open the call's wait history and hand
//     over to search.hip / search_binary.hip; mqvs_merge_shards,
//     mqvs_generate_device and mqvs_measure_read_bandwidth.
// Workspaces and their HBM gate are in workspace.hip, the host waits in
// wait.hip, segments and the column ingest in segment.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>

#include "workspace.h"


namespace mqvs {

static thread_local std::string g_error;
static thread_local mqvs_search_stats g_stats{};
// Process-wide defaults of the per-call mode flags (mqvs_set_*): atomics, read
// once at the entry of a call, so a setter racing with searches on other
// threads never switches a search's path midway (per-call flags override them).
static std::atomic<int> g_timing{0};
static std::atomic<size_t> g_scratch_budget{(size_t)1 << 30};  // bytes per scratch buffer of one call
static std::atomic<int> g_batch_mode{0};   // 0: bf16 pre-filter + exact re-rank when possible, 1: fp32 MFMA
static std::atomic<int> g_gather_mode{1};  // selective PREWHERE: 0 never gather, 1 when <= 60% selected, 2 always

size_t scratch_budget() { return g_scratch_budget.load(std::memory_order_relaxed); }
int call_batch_mode(uint32_t flags) {
    return (flags & MQVS_F_EXACT) ? 1 : g_batch_mode.load(std::memory_order_relaxed);
}
int call_gather_mode(uint32_t flags) {
    if (flags & MQVS_F_GATHER_NEVER) return 0;
    if (flags & MQVS_F_GATHER_ALWAYS) return 2;
    return g_gather_mode.load(std::memory_order_relaxed);
}
bool timing_on(uint32_t flags) { return (flags & MQVS_F_TIMING) || g_timing.load(std::memory_order_relaxed) != 0; }

void set_error(const std::string &msg) { g_error = msg; }
mqvs_search_stats &search_stats() { return g_stats; }

static thread_local int t_fault_status = MQVS_OK, t_fault_calls = 0;
static thread_local bool t_fault_mid = false;  // MQVS_FAULT_MID_CALL: fire inside the call instead

void fault_point() {
    if (t_fault_calls <= 0 || t_fault_mid) return;
    --t_fault_calls;
    fail(t_fault_status, "injected fault (mqvs_inject_fault)");
}

// the mid-call drill point: a filtered mqvs_search right after its
// selected-row count is queued (the count kernel is then still in flight)
void fault_point_mid() {
    if (t_fault_calls <= 0 || !t_fault_mid) return;
    --t_fault_calls;
    fail(t_fault_status, "injected fault (mqvs_inject_fault, mid-call)");
}

// An attribute of the current device, read once per device into the caller's
// table (a device past the table is asked every time).
using AttrCache = std::atomic<int>[64];
static int cached_attribute(AttrCache &cache, hipDeviceAttribute_t attr) {
    int dev = 0;
    MQVS_HIP(hipGetDevice(&dev));
    const bool slot = dev >= 0 && dev < 64;
    int v = slot ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (v <= 0) {
        MQVS_HIP(hipDeviceGetAttribute(&v, attr, dev));
        if (slot) cache[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

int device_cus() {
    static AttrCache cache;
    return cached_attribute(cache, hipDeviceAttributeMultiprocessorCount);
}

int64_t device_lds_bytes() {
    static AttrCache cache;
    return cached_attribute(cache, hipDeviceAttributeMaxSharedMemoryPerBlock);
}

}  // namespace mqvs

using namespace mqvs;

// ---------------------------------------------------------------------------
extern "C" {

int mqvs_abi_version(void) { return MQVS_ABI_VERSION; }

const char *mqvs_last_error(void) { return g_error.c_str(); }

int mqvs_init(int device) {
    return guarded([&] {
        int n = 0;
        MQVS_HIP(hipGetDeviceCount(&n));
        if (device < 0 || device >= n) fail(MQVS_ERR_BAD_ARGUMENTS, "no such device");
        MQVS_HIP(hipSetDevice(device));
    });
}

int mqvs_device_count(int *count) {
    return guarded([&] {
        if (!count) fail(MQVS_ERR_BAD_ARGUMENTS, "null count");
        MQVS_HIP(hipGetDeviceCount(count));
    });
}

int mqvs_thread_release(void) {
    return guarded([&] {
        index_thread_release();
        release_thread_workspaces();
    });
}

int mqvs_shutdown(void) { return mqvs_thread_release(); }

int mqvs_inject_fault(int32_t status, int32_t calls) {
    const bool mid = (status & MQVS_FAULT_MID_CALL) != 0;
    status &= ~MQVS_FAULT_MID_CALL;
    if (calls < 0 || (calls > 0 && status != MQVS_ERR_DEVICE && status != MQVS_ERR_MEMORY_LIMIT)) {
        set_error("mqvs_inject_fault: status must be MQVS_ERR_DEVICE or MQVS_ERR_MEMORY_LIMIT, calls >= 0");
        return MQVS_ERR_BAD_ARGUMENTS;
    }
    t_fault_status = status;
    t_fault_calls = calls;
    t_fault_mid = mid;
    return MQVS_OK;
}

int mqvs_search_ex(mqvs_segment_t seg, const float *queries, int32_t nq, int32_t k, int32_t metric,
                   const uint8_t *filter, const uint8_t *row_exists, int64_t chunk_ord_base,
                   int64_t *out_ids, float *out_dist, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        if (chunk_ord_base > INT32_MAX) fail(MQVS_ERR_BAD_ARGUMENTS, "chunk_ord_base out of range");
        WaitScope wsc{1, (uint64_t)(uintptr_t)seg, (uint64_t)nq, (uint64_t)k, (uint64_t)metric, filter != nullptr,
                      row_exists != nullptr, flags};
        search_internal(seg, queries, nq, k, metric, filter, row_exists, out_ids, out_dist, flags,
                        (hipStream_t)stream, chunk_ord_base);
    });
}

// (base -1: every earlier chunk of the part searched)
int mqvs_search(mqvs_segment_t seg, const float *queries, int32_t nq, int32_t k, int32_t metric,
                const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                uint32_t flags, mqvs_stream_t stream) {
    return mqvs_search_ex(seg, queries, nq, k, metric, filter, row_exists, -1, out_ids, out_dist, flags, stream);
}

int mqvs_search_binary(mqvs_segment_t seg, const uint8_t *queries, int32_t nq, int32_t k, int32_t metric,
                       const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                       uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{2, (uint64_t)(uintptr_t)seg, (uint64_t)nq, (uint64_t)k, (uint64_t)metric, filter != nullptr,
                      row_exists != nullptr, flags};
        search_binary(seg, queries, nq, k, metric, filter, row_exists, out_ids, out_dist, flags,
                           (hipStream_t)stream);
    });
}

int mqvs_rerank(mqvs_segment_t seg, const float *queries, int32_t nq, const int64_t *cand,
                int32_t ncand, int32_t k, int32_t metric, const uint8_t *row_exists, int64_t *out_ids,
                float *out_dist, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        WaitScope wsc{3, (uint64_t)(uintptr_t)seg, (uint64_t)nq, (uint64_t)ncand, (uint64_t)k, (uint64_t)metric,
                      row_exists != nullptr, flags};
        rerank_flat(seg, queries, nq, cand, ncand, k, metric, row_exists, out_ids, out_dist, flags,
                    (hipStream_t)stream);
    });
}

int mqvs_merge_shards(int32_t nshards, int32_t nq, int32_t k, int32_t metric, const int64_t *in_ids,
                      const float *in_dist, int64_t *out_ids, float *out_dist, uint32_t flags,
                      mqvs_stream_t stream) {
    return guarded([&] {
        if (nshards <= 0 || nq < 0 || k < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if ((int64_t)nshards * k > ((int64_t)1 << 20)) fail(MQVS_ERR_BAD_ARGUMENTS, "nshards * k above 2^20");
        if (nq == 0 || k == 0) return;
        DeviceCall c((hipStream_t)stream);
        Workspace &ws = c.ws;
        hipStream_t s = c.s;
        const size_t nin = (size_t)nshards * nq * k, nout = (size_t)nq * k;
        const int64_t *di = in_ids;
        const float *dd = in_dist;
        int64_t *oi = out_ids;
        float *od = out_dist;
        const bool devp = flags & MQVS_F_DEVICE_PTRS;
        if (!devp) {
            auto *b = (char *)ws.misc.get(nin * 12 + nout * 12 + 64);
            auto *bi = (int64_t *)b;
            auto *bd = (float *)(b + nin * 8);
            oi = (int64_t *)(b + nin * 12 + 16 - (nin * 12) % 16);
            od = (float *)((char *)oi + nout * 8);
            MQVS_HIP(hipMemcpyAsync(bi, in_ids, nin * 8, hipMemcpyHostToDevice, s));
            MQVS_HIP(hipMemcpyAsync(bd, in_dist, nin * 4, hipMemcpyHostToDevice, s));
            di = bi;
            dd = bd;
        }
        // binary distances (Hamming, Jaccard) are ascending finite values: the L2 order
        const int order = (metric == MQVS_METRIC_HAMMING || metric == MQVS_METRIC_JACCARD) ? MQVS_METRIC_L2 : metric;
        uint4 *scratch = (int64_t)nshards * k > kSortCap
                             ? (uint4 *)ws.large.get(sizeof(uint4) * 2 * (size_t)nshards * k * nq)
                             : nullptr;
        launch_merge_shards(nshards, nq, k, order, di, dd, oi, od, (flags & MQVS_F_PART_MERGE) != 0, scratch, s);
        MQVS_HIP(hipGetLastError());
        if (!devp) {
            MQVS_HIP(hipMemcpyAsync(out_ids, oi, nout * 8, hipMemcpyDeviceToHost, s));
            MQVS_HIP(hipMemcpyAsync(out_dist, od, nout * 4, hipMemcpyDeviceToHost, s));
        }
        if (!(devp && (flags & MQVS_F_ASYNC))) host_wait(s);
    });
}

int mqvs_generate_device(uint64_t seed, int32_t mode, int64_t row0, int64_t n, int32_t d,
                         float *dev_out, mqvs_stream_t stream) {
    return guarded([&] {
        if (mode < 0 || mode > 3 || n < 0 || d <= 0) fail(MQVS_ERR_BAD_ARGUMENTS, "bad arguments");
        DeviceCall c((hipStream_t)stream);
        launch_generate(seed, mode, row0, n, d, dev_out, c.s);
        MQVS_HIP(hipGetLastError());
        host_wait(c.s);
    });
}

int mqvs_last_search_stats(mqvs_search_stats *out) {
    if (!out) return MQVS_ERR_BAD_ARGUMENTS;
    *out = g_stats;
    return MQVS_OK;
}

int mqvs_set_batch_mode(int mode) {
    if (mode != 0 && mode != 1) return MQVS_ERR_BAD_ARGUMENTS;
    g_batch_mode.store(mode);
    return MQVS_OK;
}

int mqvs_measure_read_bandwidth(size_t bytes, int32_t reps, double *gbs, double *best_ms) {
    return guarded([&] {
        if (!gbs || bytes < ((size_t)1 << 20) || reps < 1) fail(MQVS_ERR_BAD_ARGUMENTS, "bad read-sweep arguments");
        hipStream_t s = nullptr;
        MQVS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        try {
            *gbs = measure_read_sweep(bytes, reps, s, best_ms);
        } catch (...) {
            (void)hipStreamDestroy(s);
            throw;
        }
        MQVS_HIP(hipStreamDestroy(s));
    });
}

size_t mqvs_set_scratch_budget(size_t bytes) {
    if (bytes == 0) return g_scratch_budget.load();
    return g_scratch_budget.exchange(std::max<size_t>(bytes, (size_t)1 << 20));
}

int mqvs_set_gather_mode(int mode) {
    if (mode < 0 || mode > 2) return MQVS_ERR_BAD_ARGUMENTS;
    g_gather_mode.store(mode);
    return MQVS_OK;
}

int mqvs_set_timing(int enabled) {
    g_timing.store(enabled ? 1 : 0);
    return MQVS_OK;
}

}  // extern "C"
