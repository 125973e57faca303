// wait.hip -- how a calling thread waits for its GPU work: host_wait, the wait
// mode (mqvs_set_wait_mode) and the per-call wait histories (WaitScope).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <thread>

#include "mqvs_internal.h"

namespace mqvs {

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

// this thread's last two waits (us) per wait key: (call shape, position in
// the call), 16 keys, least recently used out
struct WaitHist {
    uint64_t key;
    double h[2];
    uint64_t used;
};

// the history of the wait about to be made (the next position of the current
// WaitScope's call), marked as the most recently used
static WaitHist *wait_history() {
    static thread_local WaitHist t_tab[16];
    static thread_local uint64_t t_use = 0;
    const uint64_t key = t_wait_key ? wait_mix(t_wait_key, (uint64_t)t_wait_ord++) | 1 : 1;
    WaitHist *hs = nullptr;
    for (WaitHist &e : t_tab)
        if (e.key == key) hs = &e;
    if (!hs) {
        hs = &t_tab[0];
        for (WaitHist &e : t_tab)
            if (e.used < hs->used) hs = &e;
        *hs = WaitHist{key, {0.0, 0.0}, 0};
    }
    hs->used = ++t_use;
    return hs;
}

void host_wait(hipStream_t s) {
    const int spin = wait_spin_us();
    if (spin < 0) {
        MQVS_HIP(hipStreamSynchronize(s));
        return;
    }
    using clk = std::chrono::steady_clock;
    static thread_local double t_late = 60.0;  // how late this thread's sleeps wake (us)
    WaitHist *hs = wait_history();
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

}  // namespace mqvs

using namespace mqvs;

extern "C" int mqvs_set_wait_mode(int mode, int spin_us) {
    if (mode < MQVS_WAIT_RUNTIME || mode > MQVS_WAIT_BLOCK) {
        set_error("mqvs_set_wait_mode: mode must be MQVS_WAIT_RUNTIME, MQVS_WAIT_HYBRID or MQVS_WAIT_BLOCK");
        return -MQVS_ERR_BAD_ARGUMENTS;
    }
    if (spin_us >= 0) g_wait_spin_us.store(spin_us);
    return g_wait_mode.exchange(mode);
}
