// mqvs.hip -- C-ABI of libmqvs.so: segments, workspaces, search orchestration.
//
// Search = the whole of MergeTreeVSManager::vectorScanWithoutIndex for one data
// part (MergeTreeVSManager.cpp:960-1536) in a handful of launches:
//   1. query prep        (norms; cosine re-normalisation variants)
//   2. probe scan        dense values for rows [0, P) (P ~ 3k*n/4096)
//   3. probe select      per-query k-th key -> threshold tau; first candidates
//   4. main scan         rows [P, n), append rows with key <= tau
//   5. final select      sort candidates by the reference's total order, emit k
// If a candidate list overflows (adversarial ties), tau is tightened from the
// stored candidates and the part is re-scanned (rare; counted in the stats).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "workspace.h"


namespace mqvs {

static thread_local std::string g_error;
static thread_local mqvs_search_stats g_stats{};
// Process-wide defaults of the per-call mode flags (mqvs_set_*): atomics, read
// once at the entry of a call, so a setter racing with searches on other
// threads never switches a search's path midway (per-call flags override them).
static std::atomic<int> g_timing{0};
static std::atomic<int> g_prefilter{2};  // planes built by new segments (mqvs_set_prefilter)
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

// ---------------------------------------------------------------------------
// Workspace HBM budget (mqvs_set_workspace_budget).  The reference admits up
// to 2 x physical cores concurrent scans (MergeTreeVSManager.cpp:972-975,
// ScanThreadLimiter.h:25-58), each of which here keeps a per-thread device
// workspace (~1 GB at nq 1000).  A call is admitted with a reservation of
// the workspace it is expected to grow to (its thread's last call, or the last
// call of any thread); when that would take the sum of all workspaces and
// reservations past the budget, idle workspaces (threads between calls) are
// freed first, then the call waits until running calls finish and give their
// memory back (a call that ends while others wait frees its workspace).
// Growth beyond the reservation passes the same gate inside the call; only
// if every running call is then waiting does it go over the budget (counted)
// rather than deadlock.

struct WsGate {
    std::mutex mu;
    std::condition_variable cv;
    size_t held = 0, peak = 0;  // device bytes of all workspaces
    size_t reserved = 0;        // admitted calls' expected growth not yet allocated
    size_t typical = 0;         // the last finished call's workspace (a new thread's estimate)
    int active = 0;             // threads inside a call
    int blocked = 0;            // of them, waiting for memory
    int admitting = 0;          // threads waiting to start a call
    int trimming = 0;           // workspaces being freed outside the mutex (their bytes still in held)
    int64_t waits = 0, trims = 0, over = 0;
    std::vector<Workspace *> all;
};
static WsGate &gate() {
    static WsGate *g = new WsGate();  // (leaked: workspaces of exited threads stay registered)
    return *g;
}
static std::atomic<size_t> g_ws_budget{0};  // 0 = not set: a quarter of the device's memory, fixed at first use
static size_t ws_budget() {
    size_t b = g_ws_budget.load(std::memory_order_relaxed);
    if (b) return b;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || tot == 0) tot = (size_t)64 << 30;
    b = tot / 4;
    size_t expect = 0;
    g_ws_budget.compare_exchange_strong(expect, b);
    return g_ws_budget.load(std::memory_order_relaxed);
}

void Workspace::init(int dev) {
    if (stream) return;
    device = dev;
    MQVS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (auto &e : ev) MQVS_HIP(hipEventCreate(&e));
    for (auto &e : seg_ev) MQVS_HIP(hipEventCreate(&e));
    MQVS_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    MQVS_HIP(hipHostMalloc((void **)&host_flags, 64 * sizeof(int), hipHostMallocDefault));
    WsGate &g = gate();
    std::lock_guard<std::mutex> lk(g.mu);
    g.all.push_back(this);
}

size_t Workspace::free_buffers(bool keep_sticky) {
    size_t b = io.release();
    for (GBuf *x : {&qvars, &qnorms, &qmu, &qlam, &status, &ord, &probe, &tau, &count, &cand, &overflow, &misc, &qhi,
                    &bq, &thr, &cand2, &count2, &gcount, &goff, &glist, &large, &sticky, &surv, &recs, &flags, &p4q,
                    &qord, &pg_q, &pg_qvars, &pg_slots, &pg_bits, &pg_matrix, &pg_lists, &pg_sort, &pg_part}) {
        if (keep_sticky && x == &sticky) continue;
        b += x->cap;
        x->release();
    }
    pg_pin_in.release();
    pg_pin_out.release();
    return b;
}

// free every buffer but the ASYNC sticky word (and the index scratch
// counted here), once the last call's work has drained -- on whichever
// stream it ran, the caller's included (an ASYNC call returns with its
// kernels in flight).  Called WITHOUT the gate mutex (GPU waits and frees
// must not stall every other thread's admission) by a thread that holds
// `use`; the caller updates `held` and the gate under the mutex.
size_t Workspace::trim() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    (void)hipEventSynchronize(done);
    (void)hipStreamSynchronize(stream);
    size_t b = free_buffers(true);
    if (ext) b += ext->free_scratch();
    if (cur >= 0) (void)hipSetDevice(cur);
    return b;
}

void Workspace::release() {
    {
        WsGate &g = gate();
        std::lock_guard<std::mutex> lk(g.mu);
        g.all.erase(std::remove(g.all.begin(), g.all.end(), this), g.all.end());
        g.held -= std::min(g.held, held);
        held = 0;
    }
    if (ext) (void)ext->free_scratch();
    ext = nullptr;
    (void)free_buffers(false);
    if (host_flags) (void)hipHostFree(host_flags);
    host_flags = nullptr;
    for (auto &e : ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : seg_ev)
        if (e) (void)hipEventDestroy(e);
    if (done) (void)hipEventDestroy(done);
    done = nullptr;
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
}

// lk holds the gate mutex: free idle workspaces of other threads until `need`
// more bytes fit under the budget.  The victims are picked (their `use` taken,
// marked) under the mutex; their GPU waits and frees run with it released, and
// the accounting is updated once it is re-taken.  Returns whether anything was
// trimmed (the caller re-checks its condition either way).
static bool trim_idle(std::unique_lock<std::mutex> &lk, WsGate &g, Workspace *me, size_t need, size_t budget) {
    std::vector<Workspace *> victims;
    size_t expect = 0;
    for (Workspace *w : g.all) {
        if (g.held - std::min(g.held, expect) + g.reserved + need <= budget) break;
        if (w == me || w->trimming || w->held <= w->sticky.cap || !w->use.try_lock()) continue;
        w->trimming = true;
        victims.push_back(w);
        expect += w->held - w->sticky.cap;
    }
    if (victims.empty()) return false;
    g.trimming += (int)victims.size();
    lk.unlock();
    for (Workspace *w : victims) (void)w->trim();
    lk.lock();
    for (Workspace *w : victims) {
        // (the gate counted held - sticky of it: every gated buffer is gone)
        g.held -= std::min(g.held, w->held - std::min(w->held, w->sticky.cap));
        w->held = std::min(w->held, w->sticky.cap);
        w->trimming = false;
        ++g.trims;
        --g.trimming;
        w->use.unlock();
    }
    g.cv.notify_all();
    return true;
}

void *Workspace::grow(DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (bytes <= b.cap) return b.p;
    const size_t old = b.cap, delta = bytes - old;
    {
        WsGate &g = gate();
        std::unique_lock<std::mutex> lk(g.mu);
        // the admitted reservation first
        const size_t take = std::min(delta, resv);
        resv -= take;
        g.reserved -= std::min(g.reserved, take);
        const size_t rest = delta - take;
        g.held += take;
        held += take;
        if (rest) {
            const size_t B = ws_budget();
            bool counted = false;
            while (g.held + g.reserved + rest > B) {
                trim_idle(lk, g, this, rest, B);
                if (g.held + g.reserved + rest <= B) break;
                // (memory being freed outside the mutex comes back: wait for it)
                const int others = g.active - g.blocked - (depth > 0 ? 1 : 0);
                if (others <= 0 && g.trimming == 0) {
                    ++g.over;  // every running call waits: go over rather than deadlock
                    break;
                }
                if (!counted) ++g.waits;
                counted = true;
                ++g.blocked;
                g.cv.wait(lk);
                --g.blocked;
            }
            g.held += rest;
            held += rest;
        }
        call_peak = std::max(call_peak, held);
        g.peak = std::max(g.peak, g.held);
    }
    try {
        b.get(bytes);
    } catch (...) {
        // (the old buffer is gone too)
        WsGate &g = gate();
        std::lock_guard<std::mutex> lk(g.mu);
        g.held -= std::min(g.held, bytes);
        held -= std::min(held, bytes);
        g.cv.notify_all();
        throw;
    }
    return b.p;
}

// WsCall (workspace.h).  The thread's current call: the innermost WsCall's
// workspace, through whose gate GBufs grow
static thread_local Workspace *t_current = nullptr;

WsCall::WsCall(Workspace &w) : ws(w), prev_(t_current) {
    t_current = &ws;
    if (ws.depth++ != 0) return;
    ws.use.lock();
    WsGate &g = gate();
    std::unique_lock<std::mutex> lk(g.mu);
    // admission: reserve the expected workspace
    const size_t B = ws_budget();
    const size_t need = std::max(ws.recent ? ws.recent : g.typical, ws.held);
    const size_t extra = need - ws.held;
    bool counted = false;
    while (g.held + g.reserved + extra > B) {
        trim_idle(lk, g, &ws, extra, B);
        // (nobody to wait for: no running call, no trim in flight)
        if (g.held + g.reserved + extra <= B || (g.active == 0 && g.trimming == 0)) break;
        if (!counted) ++g.waits;
        counted = true;
        ++g.admitting;
        g.cv.wait(lk);
        --g.admitting;
    }
    ++g.active;
    ws.resv = extra;
    g.reserved += extra;
    ws.call_peak = ws.held;
}
WsCall::~WsCall() {
    t_current = prev_;
    if (--ws.depth != 0) return;
    (void)hipEventRecord(ws.done, ws.last ? ws.last : ws.stream);
    ws.last = nullptr;
    WsGate &g = gate();
    bool self_trim = false;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        --g.active;
        g.reserved -= std::min(g.reserved, ws.resv);
        ws.resv = 0;
        ws.recent = ws.call_peak;
        g.typical = ws.call_peak;
        const size_t B = g_ws_budget.load(std::memory_order_relaxed);
        self_trim = (g.blocked > 0 || g.admitting > 0 || (B && g.held > B)) && ws.held > ws.sticky.cap &&
                    hipEventQuery(ws.done) == hipSuccess;
        if (self_trim) ++g.trimming;  // (waiters wait for these bytes instead of going over)
        g.cv.notify_all();
    }
    if (self_trim) {
        // (the frees run outside the gate mutex; `use` is still held, so
        // no trimmer picks this workspace meanwhile)
        (void)ws.trim();
        std::lock_guard<std::mutex> lk(g.mu);
        g.held -= std::min(g.held, ws.held - std::min(ws.held, ws.sticky.cap));
        ws.held = std::min(ws.held, ws.sticky.cap);
        ++g.trims;
        --g.trimming;
        g.cv.notify_all();
    }
    ws.use.unlock();
}

static thread_local std::map<int, Workspace> *g_ws = nullptr;

Workspace &workspace(int device) {
    if (!g_ws) g_ws = new std::map<int, Workspace>();  // leaked at exit on purpose
    Workspace &w = (*g_ws)[device];
    w.init(device);
    return w;
}

// WsScope (mqvs_internal.h): a WsCall on the thread's workspace for the files
// that do not see Workspace (index.hip), with their scratch attached to it
WsScope::WsScope(int device, WsExt *ext) {
    Workspace &w = workspace(device);
    call_ = new WsCall(w);  // admission (may wait for memory)
    w.ext = ext;            // (one ext per thread and device; `use` is held)
}
WsScope::~WsScope() { delete static_cast<WsCall *>(call_); }
void WsScope::set_stream(hipStream_t s) { static_cast<WsCall *>(call_)->ws.last = s; }

void *GBuf::get(size_t bytes) {
    if (!t_current) fail(MQVS_ERR_LOGICAL, "gated scratch grown outside a workspace scope");
    return t_current->grow(*this, bytes);
}

int *sticky_word(Workspace &ws, hipStream_t s) {
    if (!ws.sticky.p) {
        ws.grow(ws.sticky, 16);
        MQVS_HIP(hipMemsetAsync(ws.sticky.p, 0, 16, s));
    }
    return (int *)ws.sticky.p;
}

int *async_sticky(int device, hipStream_t s) { return sticky_word(workspace(device), s); }

void ws_detach_ext(int device, WsExt *ext) {
    if (!g_ws) return;
    auto it = g_ws->find(device);
    if (it == g_ws->end()) return;
    Workspace &w = it->second;
    std::lock_guard<std::mutex> u(w.use);
    if (w.ext != ext) return;
    const size_t b = ext->free_scratch();
    WsGate &g = gate();
    std::lock_guard<std::mutex> lk(g.mu);
    g.held -= std::min(g.held, b);
    w.held -= std::min(w.held, b);
    w.ext = nullptr;
    g.cv.notify_all();
}

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

// ---------------------------------------------------------------------------
// Host waits (mqvs_set_wait_mode).  The reference admits up to 2 x physical
// cores concurrent scans (ScanThreadLimiter.h:25-58, MergeTreeVSManager.cpp:
// 974-975); here each of them waits for its GPU work, and a waiting thread
// that spins holds a host core for the whole search.  On ROCm neither
// hipStreamSynchronize nor hipEventSynchronize on a hipEventBlockingSync
// event sleeps (the runtime documents BlockingSync as a synonym of Yield;
// measured: thread CPU time = wall time in every runtime mode,
// profiles/r06/host_cpu_wait_runtime.jsonl), so the library sleeps itself:
// HYBRID polls the work's completion event for up to spin_us (a short
// search returns without a wake-up), then sleeps most of the time this
// thread's recent waits took (the shorter of the last two: searches of one
// thread are alike, and a shorter one must not wait behind a longer one's
// estimate): to 97 % of it, then polls through its end (at most a tenth of
// it), then -- a first wait, or a longer one -- polls with sleeps of 1/32 of
// the time waited so far (10-200 us: the overshoot stays a few per cent of
// the wait).  Sleeps are shortened by how late this thread's wake-ups have
// landed; a wait found done on waking halves the estimate, so the estimate
// never learns the sleep's overshoot; an expected wait under 3 wake-up
// latenesses is polled through (a sleep cannot save much of it), and in
// HYBRID so is one under 10 spin_us.  The history
// is kept per call shape and wait position (WaitScope): one history for every
// call made nq 1 searches after nq 1000 ones sleep 13 ms for 2.4 ms of work.
// BLOCK skips both polls.
static std::atomic<int> g_wait_mode{MQVS_WAIT_HYBRID};
static std::atomic<int> g_wait_spin_us{50};

void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}

int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    MQVS_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) {
        int cus = 0;
        MQVS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        return cus;
    }
    int cus = cache[dev].load(std::memory_order_relaxed);
    if (cus <= 0) {
        MQVS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        cache[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

int64_t device_lds_bytes() {
    static std::atomic<int> cache[64];
    int dev = 0;
    MQVS_HIP(hipGetDevice(&dev));
    int lds = (dev >= 0 && dev < 64) ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (lds <= 0) {
        MQVS_HIP(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        if (dev >= 0 && dev < 64) cache[dev].store(lds, std::memory_order_relaxed);
    }
    return lds;
}

int wait_spin_us() {
    const int m = g_wait_mode.load(std::memory_order_relaxed);
    return m == MQVS_WAIT_RUNTIME ? -1 : m == MQVS_WAIT_BLOCK ? 0 : g_wait_spin_us.load(std::memory_order_relaxed);
}

// one completion event per thread and device (the current one)
static hipEvent_t wait_event() {
    struct Events {
        std::map<int, hipEvent_t> ev;
        ~Events() {
            for (auto &e : ev) (void)hipEventDestroy(e.second);
        }
    };
    static thread_local Events t_ev;
    int dev = 0;
    MQVS_HIP(hipGetDevice(&dev));
    hipEvent_t &e = t_ev.ev[dev];
    if (!e) MQVS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return e;
}

static thread_local uint64_t t_wait_key = 0;  // the current API call's shape (0: none)
static thread_local int t_wait_ord = 0;        // waits so far in that call

static uint64_t wait_mix(uint64_t h, uint64_t v) {
    h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    return h * 0xFF51AFD7ED558CCDull;
}

WaitScope::WaitScope(std::initializer_list<uint64_t> parts) : prev_key(t_wait_key), prev_ord(t_wait_ord) {
    uint64_t h = 0x6A09E667F3BCC909ull;
    for (uint64_t v : parts) h = wait_mix(h, v);
    t_wait_key = h | 1;
    t_wait_ord = 0;
}

WaitScope::~WaitScope() {
    t_wait_key = prev_key;
    t_wait_ord = prev_ord;
}

void host_wait(hipStream_t s) {
    const int spin = wait_spin_us();
    if (spin < 0) {
        MQVS_HIP(hipStreamSynchronize(s));
        return;
    }
    using clk = std::chrono::steady_clock;
    // this thread's last two waits (us) per wait key: (call shape, position in
    // the call), 16 keys, least recently used out
    struct Hist {
        uint64_t key;
        double h[2];
        uint64_t used;
    };
    static thread_local Hist t_tab[16];
    static thread_local uint64_t t_use = 0;
    static thread_local double t_late = 60.0;  // how late this thread's sleeps wake (us)
    const uint64_t key = t_wait_key ? wait_mix(t_wait_key, (uint64_t)t_wait_ord++) | 1 : 1;
    Hist *hs = nullptr;
    for (Hist &e : t_tab)
        if (e.key == key) hs = &e;
    if (!hs) {
        hs = &t_tab[0];
        for (Hist &e : t_tab)
            if (e.used < hs->used) hs = &e;
        *hs = Hist{key, {0.0, 0.0}, 0};
    }
    hs->used = ++t_use;
    hipEvent_t e = wait_event();
    MQVS_HIP(hipEventRecord(e, s));
    const auto t0 = clk::now();
    auto since = [](clk::time_point a) { return std::chrono::duration<double, std::micro>(clk::now() - a).count(); };
    auto done = [&]() {
        const hipError_t q = hipEventQuery(e);
        if (q == hipSuccess) return true;
        if (q != hipErrorNotReady) MQVS_HIP(q);
        return false;
    };
    bool fin = done();
    auto poll_to = [&](double stop_us) {
        while (!fin && since(t0) < stop_us) {
            for (int i = 0; i < 32; ++i) cpu_relax();
            fin = done();
        }
    };
    auto nap = [&](double us) {  // sleep, learning how late the wake-up lands
        const auto a = clk::now();
        std::this_thread::sleep_for(std::chrono::microseconds((int64_t)us));
        t_late = 0.8 * t_late + 0.2 * std::min(1000.0, std::max(0.0, since(a) - us));
        fin = done();
    };
    // 1. poll (HYBRID)
    poll_to(spin);
    const double hint = std::min(hs->h[0], hs->h[1]);
    // what this wait tells the next one: the time waited, except when the
    // work was found done on waking from step 2 -- it ended somewhere before,
    // and recording the wake-up time would ratchet the estimate up by the
    // sleep's overshoot every search; halve the estimate instead (a shorter
    // search than the history's is then re-timed within two waits), and the
    // next wait's step 3 or 4 times it again
    double learned = -1;
    if (!fin && hint > 0) {
        if (spin > 0 && hint < std::max(3 * t_late, 10.0 * spin)) {
            // (HYBRID, a short wait -- under 10 spin_us, 500 us by default, or
            // 3 wake-up latenesses: polled through.  A sleep there saves
            // little CPU and its wake-up jitter is a large share of the wait:
            // 1 % of 50M rows at nq 1, 0.420 ms polled vs 0.457 ms with the
            // sleep, tools/wait_ab.py.  Under load waits grow past it.)
            poll_to(2 * hint + spin);
        } else {
            // 2. sleep to 97 % of the expected time, less the wake-up's lateness
            const double until = 0.97 * hint - t_late, now_us = since(t0);
            if (until > now_us + 20) {
                nap(until - now_us);
                if (fin) learned = std::min(since(t0), 0.5 * hint);
            }
            // 3. poll through the expected end (at most a tenth of the expected time)
            poll_to(std::min(1.1 * hint, since(t0) + 0.1 * hint));
        }
    }
    // 4. sleep-poll (a first wait, or one longer than expected)
    while (!fin) nap(std::min(200.0, std::max(10.0, since(t0) / 32)));
    // (a wait the first poll covers -- a status copy after the work, say --
    // says nothing about the next search's length)
    const double w = learned > 0 ? learned : since(t0);
    if (w > 50.0) {
        hs->h[1] = hs->h[0];
        hs->h[0] = w;
    }
}


// ---------------------------------------------------------------------------
// segments

static void prepare_segment(mqvs_segment *s, const uint8_t *dev_nonempty_bytes,
                            hipStream_t st) {
    if (dev_nonempty_bytes) {
        MQVS_HIP(hipMalloc((void **)&s->nonempty_bits, (size_t)(s->n + 7) / 8));
        s->bytes += (size_t)(s->n + 7) / 8;
        launch_pack_nonempty(dev_nonempty_bytes, s->n, s->nonempty_bits, st);
        const int64_t nchunks = (s->n + s->granule - 1) / s->granule;
        MQVS_HIP(hipMalloc((void **)&s->chunk_ord, sizeof(int) * std::max<int64_t>(nchunks, 1)));
        s->bytes += sizeof(int) * nchunks;
        launch_chunk_ordinals(nullptr, s->nonempty_bits, nullptr, s->n, s->granule, 0,
                              s->chunk_ord, st);
    }
    if (s->metric == MQVS_METRIC_COSINE) launch_normalize_rows(s->rows, s->n, s->d, st);
    // |y|^2 per row: the BLAS-branch L2 norms, and (all metrics) the bound of
    // the bf16 pre-filter
    MQVS_HIP(hipMalloc((void **)&s->norms, sizeof(float) * std::max<int64_t>(s->n, 1)));
    s->bytes += sizeof(float) * s->n;
    launch_row_norms(s->rows, s->n, s->d, s->norms, st);
    // bf16 plane of the rows for the nq >= 20 pre-filter (rows padded to kBfK)
    s->dpad = (s->d + kBfK - 1) / kBfK * kBfK;
    MQVS_HIP(hipMalloc((void **)&s->ynorm_max, 16 + sizeof(float) * kMxRec));
    MQVS_HIP(hipMemsetAsync(s->ynorm_max, 0, 16 + sizeof(float) * kMxRec, st));
    launch_max_norm(s->norms, s->n, s->ynorm_max, st);
    const int64_t nr = std::max<int64_t>(s->n, 1);
    const int64_t nr16 = (nr + 15) / 16 * 16;  // row-blocked planes: blocks of 16 rows
    const int split = g_prefilter.load(std::memory_order_relaxed);
    const size_t hb = (size_t)nr16 * s->dpad * sizeof(uint16_t);
    if (split == kHiSplit && hipMalloc((void **)&s->rows_hi, hb) == hipSuccess) {
        s->bytes += hb;
        launch_to_hi(s->rows, s->n, s->d, s->d, s->dpad, 1, nr16, s->rows_hi, nullptr, s->ynorm_max + 4, st);
        s->split = split;
        s->plane_bytes = hb;
    } else {
        (void)hipGetLastError();  // no room (or planes off): exact fp32 batch path only
        s->rows_hi = nullptr;
    }
    MQVS_HIP(hipGetLastError());
    float ymax = 0.f;
    MQVS_HIP(hipMemcpyAsync(&ymax, s->ynorm_max, sizeof(float), hipMemcpyDeviceToHost, st));
    MQVS_HIP(hipStreamSynchronize(st));
    // the bound needs finite, moderate norms (FLT_MAX-filled empty arrays of
    // L2/IP parts overflow): otherwise the exact fp32 path serves nq >= 20
    s->approx_ok = s->rows_hi != nullptr && ymax == ymax && ymax < 1e18f;
}

static void check_seg_args(int64_t n, int32_t d, int32_t metric, int64_t granule,
                           int64_t row_offset) {
    if (n < 0 || n >= ((int64_t)1 << 32)) fail(MQVS_ERR_BAD_ARGUMENTS, "segment rows must be in [0, 2^32)");
    if (d <= 0) fail(MQVS_ERR_BAD_ARGUMENTS, "dimension must be positive");
    if (metric != MQVS_METRIC_L2 && metric != MQVS_METRIC_IP && metric != MQVS_METRIC_COSINE)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Float32 Vector");
    if (granule <= 0) fail(MQVS_ERR_BAD_ARGUMENTS, "granule_rows must be positive");
    if (row_offset < 0 || row_offset % granule != 0)
        fail(MQVS_ERR_BAD_ARGUMENTS, "row_offset must be a non-negative multiple of granule_rows");
}

static mqvs_segment *new_segment(int64_t n, int32_t d, int32_t metric, int64_t granule,
                                 int64_t row_offset) {
    auto *s = new mqvs_segment();
    MQVS_HIP(hipGetDevice(&s->device));
    s->n = n;
    s->d = d;
    s->metric = metric;
    s->granule = granule;
    s->row_offset = row_offset;
    const size_t bytes = (size_t)std::max<int64_t>(n, 1) * d * sizeof(float);
    hipError_t e = hipMalloc((void **)&s->rows, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete s;
        fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of " + std::to_string(bytes) + " bytes failed");
    }
    s->bytes = bytes;
    return s;
}

static void free_segment(mqvs_segment *s) {
    if (!s) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(s->device);
    if (s->rows_host)
        (void)hipHostFree(s->rows_host);
    else if (s->rows)
        (void)hipFree(s->rows);
    if (s->norms) (void)hipFree(s->norms);
    if (s->nonempty_bits) (void)hipFree(s->nonempty_bits);
    if (s->rows_hi) (void)hipFree(s->rows_hi);
    if (s->ynorm_max) (void)hipFree(s->ynorm_max);
    if (s->chunk_ord) (void)hipFree(s->chunk_ord);
    if (s->codes) (void)hipFree(s->codes);
    if (cur >= 0) (void)hipSetDevice(cur);
    delete s;
}

static bool all_nonempty(const uint8_t *ne, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!ne[i]) return false;
    return true;
}

static mqvs_segment *new_binary_segment(int64_t n, int32_t dim_bits, int32_t metric, int64_t granule,
                                        int64_t row_offset) {
    if (n < 0 || n >= ((int64_t)1 << 32)) fail(MQVS_ERR_BAD_ARGUMENTS, "segment rows must be in [0, 2^32)");
    if (dim_bits <= 0 || dim_bits % 8 != 0)
        fail(MQVS_ERR_BAD_ARGUMENTS, "binary vector dimension must be a positive multiple of 8 bits");
    if (metric != MQVS_METRIC_HAMMING && metric != MQVS_METRIC_JACCARD)
        fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Binary Vector");
    if (granule <= 0) fail(MQVS_ERR_BAD_ARGUMENTS, "granule_rows must be positive");
    if (row_offset < 0 || row_offset % granule != 0)
        fail(MQVS_ERR_BAD_ARGUMENTS, "row_offset must be a non-negative multiple of granule_rows");
    auto *s = new mqvs_segment();
    MQVS_HIP(hipGetDevice(&s->device));
    s->binary = true;
    s->n = n;
    s->d = dim_bits;
    s->metric = metric;
    s->granule = granule;
    s->row_offset = row_offset;
    s->code_bytes = dim_bits / 8;
    s->code_words = (int)round_up((s->code_bytes + 3) / 4, 4);
    const size_t bytes = (size_t)std::max<int64_t>(n, 1) * s->code_words * 4;
    if (hipMalloc((void **)&s->codes, bytes) != hipSuccess) {
        (void)hipGetLastError();
        delete s;
        fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of " + std::to_string(bytes) + " bytes failed");
    }
    s->bytes = bytes;
    return s;
}

// rows of `nbytes` (host or device) -> zero-padded [n][words] on the device
void upload_codes(uint32_t *dst, int words, const uint8_t *src, int64_t nbytes, int64_t n, bool dev,
                         hipStream_t s) {
    if (n <= 0) return;
    MQVS_HIP(hipMemsetAsync(dst, 0, (size_t)n * words * 4, s));
    MQVS_HIP(hipMemcpy2DAsync(dst, (size_t)words * 4, src, (size_t)nbytes, (size_t)nbytes, (size_t)n,
                              dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
}


// ---------------------------------------------------------------------------
// column ingest: the compressed files of a part's Array(Float32) column,
// decoded in HBM (kernels_ingest.hip) into the rows matrix + nonempty flags of
// MergeTreeVSManager.cpp:1381-1393, then prepared like any segment.

struct IngestTmp {
    std::vector<void *> bufs;
    void *alloc(size_t bytes) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) {
            (void)hipGetLastError();
            fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of " + std::to_string(bytes) + " bytes failed");
        }
        bufs.push_back(p);
        return p;
    }
    // side stream for the block checksums (overlaps the decode; joined before
    // the status is read)
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    ~IngestTmp() {
        if (side) (void)hipStreamSynchronize(side);
        for (void *p : bufs) (void)hipFree(p);
        if (fork) (void)hipEventDestroy(fork);
        if (join) (void)hipEventDestroy(join);
        if (side) (void)hipStreamDestroy(side);
    }
};

// block table of one compressed stream; returns (blocks, decompressed bytes)
static std::pair<int64_t, int64_t> stream_table(IngestTmp &tmp, const uint8_t *dsrc, int64_t n, IngestBlock **tab,
                                                int64_t *hbuf, const char *what, hipStream_t s) {
    const int64_t maxb = n / 25 + 1;
    *tab = (IngestBlock *)tmp.alloc(sizeof(IngestBlock) * (size_t)maxb);
    int64_t *dout = (int64_t *)tmp.alloc(4 * sizeof(int64_t));
    launch_block_table(dsrc, n, *tab, maxb, dout, s);
    MQVS_HIP(hipGetLastError());
    MQVS_HIP(hipMemcpyAsync(hbuf, dout, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    host_wait(s);
    if (hbuf[2] == 2)
        fail(MQVS_ERR_NOT_IMPLEMENTED, std::string(what) + ": compression method other than LZ4 / NONE");
    if (hbuf[2])
        fail(MQVS_ERR_ILLEGAL_COLUMN, std::string(what) + ": malformed compressed block chain (CANNOT_DECOMPRESS)");
    return {hbuf[0], hbuf[1]};
}

constexpr int kBadDataChecksum = 8, kBadSizesChecksum = 16;  // status bits (decode uses 4)

static mqvs_segment *ingest_column(const uint8_t *data_bin, int64_t data_bytes, const uint8_t *sizes_bin,
                                   int64_t sizes_bytes, int64_t n, int32_t d, int32_t metric, int64_t granule,
                                   int64_t row_offset, uint32_t flags) {
    check_seg_args(n, d, metric, granule, row_offset);
    if (data_bytes < 0 || sizes_bytes < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "negative stream size");
    if ((data_bytes > 0 && !data_bin) || (sizes_bytes > 0 && !sizes_bin))
        fail(MQVS_ERR_BAD_ARGUMENTS, "null column stream");
    const bool dev = flags & MQVS_F_DEVICE_PTRS;
    mqvs_segment *seg = new_segment(n, d, metric, granule, row_offset);
    try {
        Workspace &ws = workspace(seg->device);
        WsCall ws_call(ws);
        hipStream_t s = ws.stream;
        IngestTmp tmp;
        const uint8_t *dd = data_bin, *ds = sizes_bin;
        if (!dev) {
            auto *a = (uint8_t *)tmp.alloc((size_t)data_bytes);
            auto *b = (uint8_t *)tmp.alloc((size_t)sizes_bytes);
            if (data_bytes) MQVS_HIP(hipMemcpyAsync(a, data_bin, (size_t)data_bytes, hipMemcpyHostToDevice, s));
            if (sizes_bytes) MQVS_HIP(hipMemcpyAsync(b, sizes_bin, (size_t)sizes_bytes, hipMemcpyHostToDevice, s));
            dd = a;
            ds = b;
        }
        int64_t *h = reinterpret_cast<int64_t *>(ws.host_flags + 16);
        IngestBlock *tab_s = nullptr, *tab_d = nullptr;
        const auto sz = stream_table(tmp, ds, sizes_bytes, &tab_s, h, "array sizes stream", s);
        if (sz.second != 8 * n)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "array sizes stream holds " + std::to_string(sz.second) + " bytes for " +
                                              std::to_string(n) + " rows");
        const auto dt = stream_table(tmp, dd, data_bytes, &tab_d, h, "vector data stream", s);
        if (dt.second % 4) fail(MQVS_ERR_ILLEGAL_COLUMN, "vector data stream is not a whole number of Float32");
        int *status = (int *)tmp.alloc(sizeof(int) * 4);
        MQVS_HIP(hipMemsetAsync(status, 0, sizeof(int) * 4, s));
        const bool verify = !(flags & MQVS_F_NO_CHECKSUM);
        if (verify) {  // CompressedReadBufferBase.cpp:192-196; the verdict is read before any decoded byte is used
            MQVS_HIP(hipStreamCreateWithFlags(&tmp.side, hipStreamNonBlocking));
            MQVS_HIP(hipEventCreateWithFlags(&tmp.fork, hipEventDisableTiming));
            MQVS_HIP(hipEventCreateWithFlags(&tmp.join, hipEventDisableTiming));
            MQVS_HIP(hipEventRecord(tmp.fork, s));
            MQVS_HIP(hipStreamWaitEvent(tmp.side, tmp.fork, 0));
            launch_block_checksum(ds, tab_s, sz.first, kBadSizesChecksum, status, nullptr, tmp.side);
            launch_block_checksum(dd, tab_d, dt.first, kBadDataChecksum, status, nullptr, tmp.side);
            MQVS_HIP(hipGetLastError());
            MQVS_HIP(hipEventRecord(tmp.join, tmp.side));
        }
        auto *sizes = (uint64_t *)tmp.alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(n, 1));
        launch_decode_blocks(ds, sizes_bytes, tab_s, sz.first, (uint8_t *)sizes, status, s);
        // the common case (every array has d elements) decodes straight into the rows
        const bool direct = dt.second == 4 * n * (int64_t)d;
        float *data = direct ? seg->rows : (float *)tmp.alloc((size_t)dt.second);
        launch_decode_blocks(dd, data_bytes, tab_d, dt.first, (uint8_t *)data, status, s);
        MQVS_HIP(hipGetLastError());
        const int64_t tiles = std::max<int64_t>(1, (n + 4095) / 4096);
        auto *offs = (int64_t *)tmp.alloc(sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1));
        auto *scratch = (int64_t *)tmp.alloc(sizeof(int64_t) * (size_t)tiles);
        auto *st = (int64_t *)tmp.alloc(sizeof(int64_t) * 4);
        MQVS_HIP(hipMemsetAsync(st, 0, sizeof(int64_t) * 4, s));
        if (n > 0) launch_sizes_scan(sizes, n, d, dt.second / 4, offs, scratch, st, s);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(h, st, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        int *hstatus = reinterpret_cast<int *>(h + 3);
        if (verify) MQVS_HIP(hipStreamWaitEvent(s, tmp.join, 0));
        MQVS_HIP(hipMemcpyAsync(hstatus, status, sizeof(int), hipMemcpyDeviceToHost, s));
        host_wait(s);
        if (*hstatus & (kBadSizesChecksum | kBadDataChecksum))
            fail(MQVS_ERR_CHECKSUM, std::string("Checksum doesn't match: corrupted data (") +
                                        (*hstatus & kBadSizesChecksum ? "array sizes stream" : "vector data stream") +
                                        ", CityHash128 of a compressed block)");
        if (*hstatus)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "malformed LZ4 block (CANNOT_DECOMPRESS)");
        const int64_t notd = h[0], nelem = h[1];
        if (h[2])  // (such sizes can sum to the right count modulo 2^64)
            fail(MQVS_ERR_ILLEGAL_COLUMN, std::to_string(h[2]) + " array sizes exceed the " +
                                              std::to_string(dt.second / 4) + " elements of the data stream");
        if (nelem * 4 != dt.second)
            fail(MQVS_ERR_ILLEGAL_COLUMN, "array sizes sum to " + std::to_string(nelem) + " elements, the data stream "
                                              "holds " + std::to_string(dt.second / 4));
        const uint8_t *nonempty = nullptr;
        if (!(direct && notd == 0)) {
            // ragged or empty arrays: the reference's copy loop
            const float *srcdata = data;
            if (direct) {
                auto *copy = (float *)tmp.alloc((size_t)dt.second);
                MQVS_HIP(hipMemcpyAsync(copy, data, (size_t)dt.second, hipMemcpyDeviceToDevice, s));
                srcdata = copy;
            }
            auto *ne = (uint8_t *)tmp.alloc((size_t)std::max<int64_t>(n, 1));
            launch_array_rows(srcdata, offs, sizes, n, d, seg->rows, ne, s);
            MQVS_HIP(hipGetLastError());
            nonempty = ne;
        }
        prepare_segment(seg, nonempty, s);  // synchronises the stream
    } catch (...) {
        free_segment(seg);
        throw;
    }
    return seg;
}

// ---------------------------------------------------------------------------
// services for the index path (index.hip)

hipStream_t thread_stream(int device) { return workspace(device).stream; }


mqvs_segment *segment_from_device(const float *dev_rows, int64_t n, int d, int metric, hipStream_t st) {
    mqvs_segment *s = new_segment(n, d, metric, std::max<int64_t>(n, 1), 0);
    try {
        if (n > 0)
            MQVS_HIP(hipMemcpyAsync(s->rows, dev_rows, sizeof(float) * (size_t)n * d, hipMemcpyDeviceToDevice, st));
        prepare_segment(s, nullptr, st);
    } catch (...) {
        free_segment(s);
        throw;
    }
    return s;
}

void segment_release(mqvs_segment *s) { free_segment(s); }

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
        if (!g_ws) return;
        for (auto &kv : *g_ws) {
            (void)hipSetDevice(kv.first);
            std::lock_guard<std::mutex> lk(kv.second.use);
            kv.second.release();
        }
        g_ws->clear();
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

int mqvs_segment_create(const float *host_rows, int64_t n, int32_t d, int32_t metric,
                        int64_t granule_rows, const uint8_t *nonempty, int64_t row_offset,
                        mqvs_segment_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        check_seg_args(n, d, metric, granule_rows, row_offset);
        if (n > 0 && !host_rows) fail(MQVS_ERR_BAD_ARGUMENTS, "null rows");
        mqvs_segment *s = new_segment(n, d, metric, granule_rows, row_offset);
        try {
            Workspace &ws = workspace(s->device);
            WsCall ws_call(ws);
            if (n > 0)
                MQVS_HIP(hipMemcpyAsync(s->rows, host_rows, sizeof(float) * (size_t)n * d,
                                        hipMemcpyHostToDevice, ws.stream));
            const uint8_t *dne = nullptr;
            if (nonempty && n > 0 && !all_nonempty(nonempty, n)) {
                auto *b = (uint8_t *)ws.misc.get((size_t)n);
                MQVS_HIP(hipMemcpyAsync(b, nonempty, (size_t)n, hipMemcpyHostToDevice, ws.stream));
                dne = b;
            }
            prepare_segment(s, dne, ws.stream);
        } catch (...) {
            free_segment(s);
            throw;
        }
        *out = s;
    });
}

int mqvs_segment_create_device(const float *dev_rows, int64_t n, int32_t d, int32_t metric,
                               int64_t granule_rows, const uint8_t *dev_nonempty,
                               int64_t row_offset, mqvs_segment_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        check_seg_args(n, d, metric, granule_rows, row_offset);
        if (n > 0 && !dev_rows) fail(MQVS_ERR_BAD_ARGUMENTS, "null rows");
        mqvs_segment *s = new_segment(n, d, metric, granule_rows, row_offset);
        try {
            Workspace &ws = workspace(s->device);
            WsCall ws_call(ws);
            if (n > 0)
                MQVS_HIP(hipMemcpyAsync(s->rows, dev_rows, sizeof(float) * (size_t)n * d,
                                        hipMemcpyDeviceToDevice, ws.stream));
            prepare_segment(s, dev_nonempty, ws.stream);
        } catch (...) {
            free_segment(s);
            throw;
        }
        *out = s;
    });
}

int mqvs_segment_generate(uint64_t seed, int32_t mode, int64_t n, int32_t d, int32_t metric,
                          int64_t granule_rows, int64_t row_offset, mqvs_segment_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        check_seg_args(n, d, metric, granule_rows, row_offset);
        if (mode < 0 || mode > 3) fail(MQVS_ERR_BAD_ARGUMENTS, "generator mode must be 0, 1, 2 or 3");
        mqvs_segment *s = new_segment(n, d, metric, granule_rows, row_offset);
        try {
            Workspace &ws = workspace(s->device);
            WsCall ws_call(ws);
            launch_generate(seed, mode, row_offset, n, d, s->rows, ws.stream);
            MQVS_HIP(hipGetLastError());
            prepare_segment(s, nullptr, ws.stream);
        } catch (...) {
            free_segment(s);
            throw;
        }
        *out = s;
    });
}

int mqvs_segment_free(mqvs_segment_t seg) {
    return guarded([&] { free_segment(seg); });
}

int mqvs_segment_info(mqvs_segment_t seg, int64_t *n, int32_t *d, int32_t *metric,
                      int64_t *granule_rows, int64_t *row_offset, size_t *hbm_bytes) {
    return guarded([&] {
        if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
        if (n) *n = seg->n;
        if (d) *d = seg->d;
        if (metric) *metric = seg->metric;
        if (granule_rows) *granule_rows = seg->granule;
        if (row_offset) *row_offset = seg->row_offset;
        if (hbm_bytes) *hbm_bytes = seg->bytes;
    });
}

int mqvs_segment_prefilter(mqvs_segment_t seg, int32_t *split, size_t *plane_bytes, int32_t *approx_ok) {
    return guarded([&] {
        if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
        const bool planes = !seg->binary && seg->rows_hi != nullptr;
        if (split) *split = planes ? seg->split : 0;
        if (plane_bytes) *plane_bytes = planes ? seg->plane_bytes : 0;
        if (approx_ok) *approx_ok = !seg->binary && seg->approx_ok ? 1 : 0;
    });
}

int mqvs_segment_set_rows_host(mqvs_segment_t seg, int32_t host) {
    return guarded([&] {
        if (!seg) fail(MQVS_ERR_BAD_ARGUMENTS, "null segment");
        if (seg->binary) fail(MQVS_ERR_LOGICAL, "binary segment has no Float32 rows");
        if ((host != 0) == (seg->rows_host != nullptr)) return;
        DeviceGuard guard(seg->device);
        const size_t bytes = sizeof(float) * (size_t)std::max<int64_t>(seg->n, 1) * (size_t)seg->d;
        MQVS_HIP(hipDeviceSynchronize());  // (work queued on the rows, e.g. by the segment's creation)
        if (host) {
            void *h = nullptr;
            if (hipHostMalloc(&h, bytes, hipHostMallocMapped) != hipSuccess)
                fail(MQVS_ERR_MEMORY_LIMIT, "pinned host memory for the rows (" + std::to_string(bytes) + " bytes)");
            void *dptr = nullptr;
            const hipError_t e1 = hipMemcpy(h, seg->rows, bytes, hipMemcpyDeviceToHost);
            const hipError_t e2 = e1 == hipSuccess ? hipHostGetDevicePointer(&dptr, h, 0) : e1;
            if (e2 != hipSuccess) {
                (void)hipHostFree(h);
                MQVS_HIP(e2);
            }
            (void)hipFree(seg->rows);
            seg->rows = static_cast<float *>(dptr);
            seg->rows_host = h;
            seg->bytes -= std::min(seg->bytes, bytes);
        } else {
            float *d = nullptr;
            if (hipMalloc((void **)&d, bytes) != hipSuccess)
                fail(MQVS_ERR_MEMORY_LIMIT, "HBM for the rows (" + std::to_string(bytes) + " bytes)");
            const hipError_t e = hipMemcpy(d, seg->rows_host, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(d);
                MQVS_HIP(e);
            }
            (void)hipHostFree(seg->rows_host);
            seg->rows_host = nullptr;
            seg->rows = d;
            seg->bytes += bytes;
        }
    });
}

int mqvs_segment_rows_host(mqvs_segment_t seg, int32_t *host) {
    return guarded([&] {
        if (!seg || !host) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        *host = seg->rows_host != nullptr ? 1 : 0;
    });
}

int mqvs_segment_rows(mqvs_segment_t seg, const float **dev_rows) {
    return guarded([&] {
        if (!seg || !dev_rows) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (seg->binary) fail(MQVS_ERR_LOGICAL, "binary segment has no Float32 rows");
        *dev_rows = seg->rows;
    });
}

int mqvs_search(mqvs_segment_t seg, const float *queries, int32_t nq, int32_t k, int32_t metric,
                const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{1, (uint64_t)(uintptr_t)seg, (uint64_t)nq, (uint64_t)k, (uint64_t)metric, filter != nullptr,
                      row_exists != nullptr, flags};
        search_internal(seg, queries, nq, k, metric, filter, row_exists, out_ids, out_dist, flags,
                        (hipStream_t)stream);
    });
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

int mqvs_knn_raw(const float *x, const float *y, int64_t d, int64_t k, int64_t nx, int64_t ny,
                 int32_t metric, int64_t *result_id, float *distance) {
    return guarded([&] {
        if (metric != MQVS_METRIC_L2 && metric != MQVS_METRIC_IP)
            fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Float32 Vector");
        fault_point();
        if (d <= 0 || d > INT32_MAX || k < 0 || k > INT32_MAX || nx < 0 || nx > INT32_MAX || ny < 0)
            fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if (nx == 0 || k == 0) return;
        if (ny == 0) {
            for (int64_t i = 0; i < nx * k; ++i) {
                result_id[i] = -1;
                distance[i] = metric == MQVS_METRIC_L2 ? 3.40282347e+38f : -3.40282347e+38f;
            }
            return;
        }
        mqvs_segment *s = new_segment(ny, (int)d, metric, ny, 0);
        try {
            Workspace &ws = workspace(s->device);
            WsCall ws_call(ws);
            MQVS_HIP(hipMemcpyAsync(s->rows, y, sizeof(float) * (size_t)ny * d, hipMemcpyHostToDevice,
                                    ws.stream));
            prepare_segment(s, nullptr, ws.stream);
            search_internal(s, x, (int)nx, (int)k, metric == MQVS_METRIC_IP ? kMetricIpRaw : MQVS_METRIC_L2,
                            nullptr, nullptr, result_id, distance, 0, nullptr);
        } catch (...) {
            free_segment(s);
            throw;
        }
        free_segment(s);
    });
}

int mqvs_segment_create_from_column(const uint8_t *data_bin, int64_t data_bytes, const uint8_t *sizes_bin,
                                    int64_t sizes_bytes, int64_t n, int32_t d, int32_t metric, int64_t granule_rows,
                                    int64_t row_offset, uint32_t flags, mqvs_segment_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        *out = ingest_column(data_bin, data_bytes, sizes_bin, sizes_bytes, n, d, metric, granule_rows, row_offset,
                             flags);
    });
}

int mqvs_segment_create_binary(const uint8_t *codes, int64_t n, int32_t dim_bits, int32_t metric,
                               int64_t granule_rows, int64_t row_offset, uint32_t flags, mqvs_segment_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        mqvs_segment *s = new_binary_segment(n, dim_bits, metric, granule_rows, row_offset);
        try {
            if (n > 0 && !codes) fail(MQVS_ERR_BAD_ARGUMENTS, "null codes");
            Workspace &ws = workspace(s->device);
            WsCall ws_call(ws);
            upload_codes(s->codes, s->code_words, codes, s->code_bytes, n, (flags & MQVS_F_DEVICE_PTRS) != 0,
                         ws.stream);
            MQVS_HIP(hipStreamSynchronize(ws.stream));
        } catch (...) {
            free_segment(s);
            throw;
        }
        *out = s;
    });
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

int mqvs_knn_binary_raw(const uint8_t *x, const uint8_t *y, int64_t d, int64_t k, int64_t nx, int64_t ny,
                        int32_t metric, int64_t *result_id, float *distance) {
    return guarded([&] {
        if (metric != MQVS_METRIC_HAMMING && metric != MQVS_METRIC_JACCARD)
            fail(MQVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Binary Vector");
        fault_point();
        if (d <= 0 || d % 8 != 0 || d > INT32_MAX || k < 0 || k > INT32_MAX || nx < 0 || nx > INT32_MAX ||
            ny < 0)
            fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if (nx == 0 || k == 0) return;
        if (ny == 0) {
            for (int64_t i = 0; i < nx * k; ++i) {
                result_id[i] = -1;
                if (metric == MQVS_METRIC_HAMMING)
                    reinterpret_cast<int32_t *>(distance)[i] = INT32_MAX;
                else
                    distance[i] = 3.40282347e+38f;
            }
            return;
        }
        mqvs_segment *s = new_binary_segment(ny, (int32_t)d, metric, ny, 0);
        try {
            Workspace &ws = workspace(s->device);
            WsCall ws_call(ws);
            upload_codes(s->codes, s->code_words, y, s->code_bytes, ny, false, ws.stream);
            const size_t m = (size_t)nx * k;
            auto *b = (char *)ws.misc.get(m * 12 + 16);
            auto *di = (int64_t *)b;
            auto *dd = (float *)(b + m * 8);
            auto *qd = (uint8_t *)ws.glist.get((size_t)nx * (d / 8));
            MQVS_HIP(hipMemcpyAsync(qd, x, (size_t)nx * (d / 8), hipMemcpyHostToDevice, ws.stream));
            search_binary(s, qd, (int)nx, (int)k, metric, nullptr, nullptr, di, dd, MQVS_F_DEVICE_PTRS,
                               nullptr);
            if (metric == MQVS_METRIC_HAMMING) launch_hamming_to_int(di, dd, (int64_t)m, ws.stream);
            MQVS_HIP(hipGetLastError());
            MQVS_HIP(hipMemcpyAsync(result_id, di, m * 8, hipMemcpyDeviceToHost, ws.stream));
            MQVS_HIP(hipMemcpyAsync(distance, dd, m * 4, hipMemcpyDeviceToHost, ws.stream));
            MQVS_HIP(hipStreamSynchronize(ws.stream));
        } catch (...) {
            free_segment(s);
            throw;
        }
        free_segment(s);
    });
}

int mqvs_merge_shards(int32_t nshards, int32_t nq, int32_t k, int32_t metric, const int64_t *in_ids,
                      const float *in_dist, int64_t *out_ids, float *out_dist, uint32_t flags,
                      mqvs_stream_t stream) {
    return guarded([&] {
        if (nshards <= 0 || nq < 0 || k < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if ((int64_t)nshards * k > ((int64_t)1 << 20)) fail(MQVS_ERR_BAD_ARGUMENTS, "nshards * k above 2^20");
        if (nq == 0 || k == 0) return;
        int dev = 0;
        MQVS_HIP(hipGetDevice(&dev));
        Workspace &ws = workspace(dev);
        WsCall ws_call(ws);
        hipStream_t s = stream ? (hipStream_t)stream : ws.stream;
        ws.last = s;
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
        int dev = 0;
        MQVS_HIP(hipGetDevice(&dev));
        Workspace &ws = workspace(dev);
        WsCall ws_call(ws);
        hipStream_t s = stream ? (hipStream_t)stream : ws.stream;
        ws.last = s;
        launch_generate(seed, mode, row0, n, d, dev_out, s);
        MQVS_HIP(hipGetLastError());
        host_wait(s);
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

int mqvs_set_prefilter(int split) {
    if (split != kHiSplit && split != 0) return MQVS_ERR_BAD_ARGUMENTS;
    g_prefilter.store(split);
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

size_t mqvs_set_workspace_budget(size_t bytes) {
    const size_t prev = ws_budget();
    if (bytes) {
        g_ws_budget.store(bytes, std::memory_order_relaxed);
        WsGate &g = gate();
        std::lock_guard<std::mutex> lk(g.mu);
        g.cv.notify_all();
    }
    return prev;
}

int mqvs_workspace_stats(mqvs_workspace_stats_t *out, int32_t reset_peak) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null stats");
        const size_t b = ws_budget();
        WsGate &g = gate();
        std::lock_guard<std::mutex> lk(g.mu);
        out->budget = b;
        out->held = g.held;
        out->peak = g.peak;
        out->waits = g.waits;
        out->trims = g.trims;
        out->over_budget = g.over;
        out->active = g.active;
        out->workspaces = (int32_t)g.all.size();
        if (reset_peak) {
            g.peak = g.held;
            g.waits = g.trims = g.over = 0;
        }
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

int mqvs_set_wait_mode(int mode, int spin_us) {
    if (mode < MQVS_WAIT_RUNTIME || mode > MQVS_WAIT_BLOCK) {
        set_error("mqvs_set_wait_mode: mode must be MQVS_WAIT_RUNTIME, MQVS_WAIT_HYBRID or MQVS_WAIT_BLOCK");
        return -MQVS_ERR_BAD_ARGUMENTS;
    }
    if (spin_us >= 0) g_wait_spin_us.store(spin_us);
    return g_wait_mode.exchange(mode);
}

int mqvs_async_check(mqvs_stream_t stream) {
    return guarded([&] {
        int dev = 0;
        MQVS_HIP(hipGetDevice(&dev));
        Workspace &ws = workspace(dev);
        WsCall ws_call(ws);
        hipStream_t s = stream ? (hipStream_t)stream : ws.stream;
        ws.last = s;
        host_wait(s);
        if (!ws.sticky.p) return;
        int word = 0;
        MQVS_HIP(hipMemcpy(&word, ws.sticky.p, sizeof(int), hipMemcpyDeviceToHost));
        MQVS_HIP(hipMemset(ws.sticky.p, 0, 16));
        if (word & 1)
            fail(MQVS_ERR_LOGICAL, "an ASYNC search needed its exact fallback (candidate overflow, or a query "
                                   "whose norm is NaN, infinite or at least 1e18; results invalid): "
                                   "repeat it without MQVS_F_ASYNC");
        if (word & 2)
            fail(MQVS_ERR_LOGICAL, "an ASYNC cosine search's query normalisation did not repeat within " +
                                       std::to_string(kMaxVariants) + " steps on a part of more chunks");
    });
}

}  // extern "C"
