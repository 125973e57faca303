// workspace.h -- the per-thread device workspace of the FLAT paths and the
// process-wide gate on the HBM all workspaces hold (workspace.hip).
#pragma once

#include <mutex>

#include "flat_kernels.h"
#include "search_host.h"

namespace mqvs {

// the pinned record [padded, selected, generation] of k_chunk_count (int64
// words at host_flags + kCountRec), and how long a filtered search polls it
constexpr int kCountRec = 32;
constexpr int kCountSpinUs = 200;

// One thread's scratch on one device.  Every buffer is a GBuf: it grows
// through the gate (Workspace::grow) of the thread's current WsCall.
struct Workspace {
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};
    static constexpr int kSegEv = 64;
    hipEvent_t seg_ev[kSegEv] = {};  // per main-scan segment: start, end
    CallIO io;                       // staged inputs and outputs of host-pointer calls
    GBuf qvars, qnorms, qmu, qlam, status, ord, probe, tau, count, cand, overflow, misc, qhi, bq, thr, cand2, count2,
        gcount, goff, glist, large, sticky, surv, recs, flags, p4q, qord;
    // binary searches on the i8 MFMA route (search_binary.hip): the call's
    // queries as 0/1 bytes and their popcounts (launch_bin_expand)
    GBuf bin_qplane, bin_qpop;
    // part-group searches (part_group.hip) keep their own buffers: the
    // per-part searches nested in such a call use the ones above
    GBuf pg_q, pg_qvars, pg_slots, pg_bits, pg_matrix, pg_lists, pg_sort, pg_part;
    // index-group searches (index_group.hip) share them (pg_matrix: the record regions) and add the
    // slices' centroid distances and the call's probes + record counters
    GBuf pg_cdist, pg_probes;
    HostBuf pg_pin_in, pg_pin_out;  // pinned staging: slot table + bitmaps; out_part
    int *host_flags = nullptr;  // pinned (64 ints; the selected-row count record at kCountRec)
    int64_t count_gen = 0;      // generation of the last selected-row count record asked for
    bool pending_timing = false, pending_bf16 = false;  // search_collect_stats
    int pending_seg_events = 0;
    int device = 0;
    std::mutex use;     // held by the owning thread during a call (WsCall); trimmers only try_lock it
    hipStream_t last = nullptr;  // the stream of the current call (the caller's, or `stream`)
    hipEvent_t done = nullptr;   // recorded on it at the end of every call: a trimmer waits for it
    int depth = 0;      // the owner's nested calls
    size_t held = 0;    // device bytes of the buffers (the gate's share of this workspace)
    size_t resv = 0;    // the current call's reservation left
    size_t call_peak = 0, recent = 0;  // most held during the current / the last call
    WsExt *ext = nullptr;  // the thread's index workspace: its scratch is counted and trimmed with this one
    bool trimming = false;  // picked by a trimmer, which waits and frees outside the gate mutex
    void init(int dev);
    // the buffers, sticky word included (gate accounting is the caller's)
    size_t free_buffers(bool keep_sticky);
    size_t trim();
    void release();
    // b grown to `bytes` through the gate (GBuf::get; the ASYNC sticky word
    // grows outside a call too)
    void *grow(DevBuf &b, size_t bytes);
};

// the calling thread's workspace on `device` (created on first use)
Workspace &workspace(int device);
// every workspace of the calling thread freed (mqvs_thread_release)
void release_thread_workspaces();

// one call of the owning thread on its workspace (nests): counted as running
// and made the thread's current one for GBuf growth; at the end, if other
// calls wait for memory (or the gate is over budget), the workspace is freed
// for them
struct WsCall {
    Workspace &ws;
    explicit WsCall(Workspace &w);
    ~WsCall();
    WsCall(const WsCall &) = delete;
    WsCall &operator=(const WsCall &) = delete;

   private:
    Workspace *prev_;
};

// A call on the calling thread's workspace of the current device, on the
// caller's stream or, when that is null, the workspace's own
struct DeviceCall {
    Workspace &ws;
    WsCall call;
    hipStream_t s;
    explicit DeviceCall(hipStream_t stream);
};

// ASYNC searches cannot run the host-driven fallbacks (exact re-scan after a
// pre-filter overflow, tightened re-scan, the cosine variant check): their
// device flags are OR-ed into this thread's sticky word, which
// mqvs_async_check reads and clears.
int *sticky_word(Workspace &ws, hipStream_t s);

// ---------------------------------------------------------------------------
// shared by search.hip and search_binary.hip

// per-stage times of the search just synchronised (HIP events on its stream);
// seg_events: the main-scan segments whose start / end events were recorded
// (0: main_ms is the whole span between the probe select and the final select)
void read_search_times(Workspace &ws, mqvs_search_stats &st, int seg_events);

// The host-driven answer to a candidate-list overflow: one main-scan segment
// held more than cap rows at or under its threshold -- a mass tie, or a part
// whose rows come ever nearer to the queries, where almost every row passes
// the threshold of the rows before it.  When the overflow word read into
// ws.host_flags[0] is set, the lists are emptied, tau is reset to "every row"
// and the part is scanned once more from position 0, inclusively, in segments
// of at most cap / 2 positions (`scan(b, e, cand, count)` appends to that
// list), with an exact refinement after each; then the select again.
// (Nothing of the overflowed pass is kept, its thresholds included: they
// came from whichever cap rows happened to be stored.)  A refined list holds
// the k best rows so far and the rows within the threshold's slack of the
// k-th (a bound: 2^-16 relative), and a segment adds at most cap / 2 rows, so
// whichever appends landed first, a list overflows again only when more than
// cap / 2 rows tie at or near a k-th key: that is the error.  One pass, no
// loop.  Returns the number of re-scans (0 or 1).
struct OverflowRescan {
    Cand *cand, *alt;  // the lists, and the buffer the refinements compact them into
    int *count, *count_alt;
    int cap, nq, k, order;  // order: the metric whose key orders the candidates
    uint32_t *tau;
    int *overflow;
    int64_t chunk_rows, id_offset;  // of the final select
    int64_t *dids;
    float *ddist;
    uint4 *large;
    int64_t rows, align;  // scan positions [0, rows); a segment's bounds are multiples of align
};
template <typename Scan>
int rescan_on_overflow(Workspace &ws, OverflowRescan r, hipStream_t s, Scan &&scan) {
    if (!ws.host_flags[0]) return 0;
    launch_fill2((uint32_t *)r.count, r.nq, 0u, (uint32_t *)r.overflow, 4, 0u, s);
    launch_fill2(r.tau, r.nq, 0xFFFFFFFEu, nullptr, 0, 0u, s);
    const int64_t seg_rows = std::max<int64_t>(r.align, r.cap / 2 / r.align * r.align);
    for (int64_t b = 0; b < r.rows; b += seg_rows) {
        const int64_t e = std::min(r.rows, b + seg_rows);
        scan(b, e, r.cand, r.count);
        if (e < r.rows) {
            launch_refine(r.cand, r.count, r.cap, r.nq, r.k, r.order, false, nullptr, r.tau, nullptr, r.alt,
                          r.count_alt, s);
            MQVS_HIP(hipGetLastError());
            std::swap(r.cand, r.alt);
            std::swap(r.count, r.count_alt);
        }
    }
    launch_final_select(r.cand, r.count, r.cap, r.nq, r.k, r.order, r.chunk_rows, r.id_offset, r.dids, r.ddist,
                        r.overflow, r.large, s);
    MQVS_HIP(hipGetLastError());
    MQVS_HIP(hipMemcpyAsync(ws.host_flags, r.overflow, sizeof(int), hipMemcpyDeviceToHost, s));
    host_wait(s);
    if (ws.host_flags[0])
        fail(MQVS_ERR_LOGICAL,
             "candidate overflow: more than " + std::to_string(r.cap) + " rows tie at the k-th distance");
    return 1;
}

}  // namespace mqvs
