// mqvs_internal.h -- the base every file of libmqvs (gfx950 only) includes:
// the segment, the tunables, the error plumbing, device buffers and the
// workspace gate's handles, and the host waits.  The FLAT kernels' interface
// is flat_kernels.h, the index kernels' index_kernels.h, and what the search
// entry points share on the host search_host.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <initializer_list>
#include <string>
#include <stdexcept>
#include <algorithm>

#include "../../include/mqvs.h"
#include "tuning.h"

struct mqvs_segment {
    int device = 0;
    int64_t n = 0;
    int d = 0;
    int metric = 0;
    int64_t granule = 0;
    int64_t row_offset = 0;
    float *rows = nullptr;           // device address (HBM, or mapped pinned host memory)
    void *rows_host = nullptr;       // the pinned host allocation when the rows live in host memory
    float *norms = nullptr;          // |y|^2 per row (fvec_norm_L2sqr order)
    uint16_t *rows_hi = nullptr;     // bf16 rounding of the rows, [n][dpad]
    float *ynorm_max = nullptr;      // device scalar: max_r |y_r|; splits 2, 6: + [kMxRec] norm maxima at +16 B
    int split = 0;                   // pre-filter planes built: 2 (bf16 hi), 0 = none
    int64_t dpad = 0;
    bool approx_ok = false;          // bf16 pre-filter usable for this segment
    size_t plane_bytes = 0;          // HBM of the pre-filter planes (0: none built)
    uint8_t *nonempty_bits = nullptr;// null when every array is non-empty
    int *chunk_ord = nullptr;        // no-filter chunk ordinals (null = identity)
    // binary segments (FixedString(N) codes; rows == nullptr)
    bool binary = false;
    uint32_t *codes = nullptr;       // [n][code_words], 16-B aligned rows, zero padded
    int code_bytes = 0;              // N = d / 8
    int code_words = 0;              // row stride in 32-bit words (multiple of 4)
    size_t bytes = 0;
};

namespace mqvs {

// ---------------------------------------------------------------------------
// Tunables
constexpr int kBlasThreshold = 20;   // faiss distance_compute_blas_threshold
constexpr int kMaxVariants = 32;     // cosine query re-normalisation variants kept (default table)
constexpr int kMaxVariantsCap = 16384;  // one variant per chunk ordinal when a chain does not repeat
constexpr int kSortCap = 4096;       // candidates sorted in LDS per query
constexpr int kMaxK = 16384;         // largest k (max_search_result_window is 10000, Settings.h:923)
constexpr int kLargeCap = 32768;     // records per query sorted through global scratch (k > kSortCap)
constexpr int64_t kCandBudget = 1 << 25;  // candidate slots per search (x 8 B)
constexpr int64_t kCandMax = 1 << 20;     // candidate slots per query
constexpr int kSmallRows = 256;      // rows per tile, VALU scan
constexpr int kMfmaRows = 128;       // rows per tile, MFMA scan
constexpr int kMfmaQ = 128;          // queries per tile, MFMA scan
constexpr int kBfRows = 256;         // rows per tile, bf16 pre-filter scans (kernels_hi.hip)
constexpr int kBfRowsSmall = 64;     // short tiles of k_scan_hi_reg (scan_hi_small_tiles_ok)
// Internal metric id: raw faiss inner product (knn_inner_product: every
// ip > -FLT_MAX enters the heap), used by mqvs_knn_raw only.  The operator
// path (mqvs_search) applies searchWrapper's FLT_MIN cut instead.
constexpr int kMetricIpRaw = 3;

// ---------------------------------------------------------------------------
// Error plumbing
void set_error(const std::string &msg);

struct Error {
    int code;
    std::string msg;
};

#define MQVS_HIP(call)                                                                 \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess)                                                          \
            throw ::mqvs::Error{e_ == hipErrorOutOfMemory ? MQVS_ERR_MEMORY_LIMIT         \
                                                          : MQVS_ERR_DEVICE,             \
                                std::string(#call) + ": " + hipGetErrorString(e_)};    \
    } while (0)

[[noreturn]] inline void fail(int code, const std::string &msg) { throw Error{code, msg}; }

template <typename F>
static int guarded(F &&f) {
    try {
        f();
        return MQVS_OK;
    } catch (const Error &e) {
        set_error(e.msg);
        return e.code;
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed");
        return MQVS_ERR_MEMORY_LIMIT;
    } catch (...) {
        set_error("unknown error");
        return MQVS_ERR_DEVICE;
    }
}

// the search entry points' fault drill (mqvs_inject_fault): throws the armed
// status while this thread's count lasts
void fault_point();
// the mid-call drill point of mqvs_inject_fault (MQVS_FAULT_MID_CALL): a
// filtered mqvs_search right after its selected-row count is queued
void fault_point_mid();

// ---------------------------------------------------------------------------
// Host-side plumbing shared by the host files: mqvs.hip (C ABI glue, modes),
// workspace.hip (the workspace gate), wait.hip (host waits), segment.hip
// (segments), search.hip and search_binary.hip (the FLAT searches), index.hip
// (the index path)

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
size_t scratch_budget();  // bytes per scratch buffer of one call (mqvs_set_scratch_budget)
// compute units of the current device (cached per device: launchers size
// their persistent grids from it on every call)
int device_cus();
// LDS bytes one workgroup of the current device can have, static + dynamic
// (hipDeviceAttributeMaxSharedMemoryPerBlock, read once per device)
int64_t device_lds_bytes();

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    void *get(size_t bytes) {
        if (bytes == 0) bytes = 16;
        if (bytes > cap) {
            if (p) (void)hipFree(p);
            p = nullptr;
            cap = 0;
            MQVS_HIP(hipMalloc(&p, bytes));
            cap = bytes;
        }
        return p;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Pinned host staging of a synchronous call's host inputs and outputs: the
// caller's (pageable) arrays are copied by the CPU into it and DMA'd from it,
// so the HIP runtime never stages a pageable copy itself (it waits for those
// by spinning: with 16 threads searching 10M x 768 at nq 1000 from host
// arrays, 18 % of each thread's wall time was CPU time, profiles/r06).
// Reused across calls (each synchronous call ends after its copies).
struct HostBuf {
    void *p = nullptr;
    size_t cap = 0;
    void *get(size_t bytes) {
        if (bytes == 0) bytes = 16;
        if (bytes > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
            MQVS_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
            cap = bytes;
        }
        return p;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Per-thread scratch of another path (the index's, index.hip) counted in, and
// trimmed with, the calling thread's FLAT workspace under the process-wide
// HBM budget (mqvs_set_workspace_budget): the reference runs index searches
// from as many part threads as FLAT scans (VIWithDataPart.cpp:900-901 under
// ScanThreadLimiter.h:25-58), so both share one admission gate.
struct WsExt {
    // every gated buffer freed once the owner's work on it has drained (the
    // caller holds the owner's workspace); returns the bytes freed
    virtual size_t free_scratch() = 0;

   protected:
    ~WsExt() = default;
};
// a DevBuf whose growth passes the gate of the calling thread's current
// workspace call (WsCall, workspace.h; WsScope below is one) -- it fails
// outside one: no ungated scratch
struct GBuf : DevBuf {
    void *get(size_t bytes);
};
// one call on the calling thread's workspace of `device` (admission, nests
// with FLAT calls), with `ext` attached to it
class WsScope {
   public:
    WsScope(int device, WsExt *ext);
    ~WsScope();
    void set_stream(hipStream_t s);  // the stream whose completion ends the call's use of its buffers
    WsScope(const WsScope &) = delete;
    WsScope &operator=(const WsScope &) = delete;

   private:
    void *call_ = nullptr;  // the WsCall
};
// index_thread_release: `ext`'s scratch freed and detached from the thread's workspace
void ws_detach_ext(int device, WsExt *ext);

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        MQVS_HIP(hipGetDevice(&prev));
        if (prev != dev) MQVS_HIP(hipSetDevice(dev));
    }
    ~DeviceGuard() {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

// ---------------------------------------------------------------------------
// Streams and host waits

// the stream of the calling thread's workspace on `device` (workspace.hip)
hipStream_t thread_stream(int device);
// The host's wait for the work queued on `s` (wait.hip; every synchronous call
// ends with one): the policy of mqvs_set_wait_mode -- the runtime's own
// hipStreamSynchronize, or a short poll of a blocking-sync event's completion
// followed by a blocking wait on it (the calling thread sleeps instead of
// holding a core for the length of the search).  The current device must be
// s's.
void host_wait(hipStream_t s);
// The wait history's key for the host_waits of one API call: set by the
// entry points from the call's shape (function, segment, nq, k, filter,
// flags); each wait position within the call keeps its own history, so a
// thread alternating nq 1000 and nq 1 searches sleeps each for its own length.
struct WaitScope {
    uint64_t prev_key;
    int prev_ord;
    explicit WaitScope(std::initializer_list<uint64_t> parts);
    ~WaitScope();
    WaitScope(const WaitScope &) = delete;
    WaitScope &operator=(const WaitScope &) = delete;
};
inline uint64_t wait_str_hash(const char *p) {  // (a parameter string's part of a wait key)
    uint64_t h = 1469598103934665603ull;
    for (; p && *p; ++p) h = (h ^ (unsigned char)*p) * 1099511628211ull;
    return h;
}
// poll budget of the hybrid wait (microseconds; 0 in MQVS_WAIT_BLOCK, -1 in
// MQVS_WAIT_RUNTIME): also bounds the spin on a pinned-memory word
int wait_spin_us();
// one pause of a host spin loop (x86 PAUSE: the core yields to its sibling
// hyper-thread and saves power while polling)
void cpu_relax();
// the call's per-kernel timing events (MQVS_F_TIMING or mqvs_set_timing)
bool timing_on(uint32_t flags);

}  // namespace mqvs
