// workspace.hip -- the per-thread device workspaces (workspace.h) and the
// process-wide gate on the HBM they hold: admission, growth, trimming, the
// ASYNC sticky word, and the C entry points of the budget.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "workspace.h"

namespace mqvs {

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
                    &qord, &pg_q, &pg_qvars, &pg_slots, &pg_bits, &pg_matrix, &pg_lists, &pg_sort, &pg_part, &pg_cdist,
                    &pg_probes, &bin_qplane, &bin_qpop}) {
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

// The gate mutex is held and w.trim() has returned: the accounting of a
// trimmed workspace (the gate counted held - sticky of it: every gated buffer
// is gone).  The caller wakes the waiters.
static void settle_trimmed(WsGate &g, Workspace &w) {
    g.held -= std::min(g.held, w.held - std::min(w.held, w.sticky.cap));
    w.held = std::min(w.held, w.sticky.cap);
    ++g.trims;
    --g.trimming;
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
        settle_trimmed(g, *w);
        w->trimming = false;
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
        settle_trimmed(g, ws);
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

void release_thread_workspaces() {
    if (!g_ws) return;
    for (auto &kv : *g_ws) {
        (void)hipSetDevice(kv.first);
        std::lock_guard<std::mutex> lk(kv.second.use);
        kv.second.release();
    }
    g_ws->clear();
}

hipStream_t thread_stream(int device) { return workspace(device).stream; }

static Workspace &current_device_workspace() {
    int dev = 0;
    MQVS_HIP(hipGetDevice(&dev));
    return workspace(dev);
}

DeviceCall::DeviceCall(hipStream_t stream)
    : ws(current_device_workspace()), call(ws), s(stream ? stream : ws.stream) {
    ws.last = s;
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

}  // namespace mqvs

using namespace mqvs;

extern "C" {

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

int mqvs_async_check(mqvs_stream_t stream) {
    return guarded([&] {
        DeviceCall c((hipStream_t)stream);
        host_wait(c.s);
        if (!c.ws.sticky.p) return;
        int word = 0;
        MQVS_HIP(hipMemcpy(&word, c.ws.sticky.p, sizeof(int), hipMemcpyDeviceToHost));
        MQVS_HIP(hipMemset(c.ws.sticky.p, 0, 16));
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
