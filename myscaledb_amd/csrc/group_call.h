// group_call.h -- what the group searches (part_group.hip, index_group.hip) do
// the same way around their grouped kernels: the argument checks and the stats
// header, the call's device, workspace and stream, the slot tables of the fused
// parts cut into slices, the call's host inputs staged with them in one copy,
// the per-part lists, and the merge with the call's one host wait.
#pragma once

#include <chrono>
#include <cstring>
#include <vector>

#include "workspace.h"

namespace mqvs {

// check_search_args, and the list index the merge writes
inline void check_group_args(const void *group, const char *what, const char *wrong_kind, int nq, int k,
                             const void *queries, const void *out_part, const void *out_ids, const void *out_dist) {
    check_search_args(group, what, wrong_kind, nq, k, queries, out_ids, out_dist);
    if (nq > 0 && k > 0 && !out_part) fail(MQVS_ERR_BAD_ARGUMENTS, "null query or output pointer");
}

// After a search's own checks: the merge's limit, then the stats header of the
// call (st, stored as the thread's last) -- all that a call with nq 0 or k 0
// leaves (false: nothing to search).
template <typename Stats>
bool group_begin(int nparts, int nq, int k, Stats &st, Stats &last) {
    if ((int64_t)nparts * k > ((int64_t)1 << 20)) fail(MQVS_ERR_BAD_ARGUMENTS, "nparts * k above 2^20");
    st = Stats{};
    st.parts = nparts;
    st.nq = nq;
    st.k = k;
    last = st;
    return nq != 0 && k != 0;
}

// The clock, device, workspace call and stream of one group search
struct GroupScope {
    const bool timing;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    DeviceGuard guard;
    Workspace &ws;
    WsCall call;
    hipStream_t s;
    GroupScope(int device, uint32_t flags, hipStream_t user_stream)
        : timing(timing_on(flags)), guard(device), ws(workspace(device)), call(ws),
          s(user_stream ? user_stream : ws.stream) {
        ws.last = s;
    }
    // host time of the call so far (0 unless timed)
    double total_ms() const {
        if (!timing) return 0.0;
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

// 16-B aligned offsets of the staged bitmaps in one buffer
inline size_t bitmap_slot(size_t &total, int64_t n) {
    const size_t off = total;
    total += (size_t)round_up((n + 7) / 8, 16);
    return off;
}

// Slot: the grouped kernels' per-part table entry (fields part, filter,
// exists).  Slice: slots [first_slot, first_slot + nslots) (+ the sentinel) of
// one grouped launch chain -- fused parts whose scratch fits the budget --
// with the running sums the slots' prefix fields come from.  rows: the rows of
// every part of the group, in group order (the bitmaps' lengths).
template <typename Slot, typename Slice>
struct GroupCall {
    const std::vector<int64_t> rows;
    Workspace &ws;
    hipStream_t s;
    bool dev;
    int nq, k;
    const uint8_t *const *filters;
    const uint8_t *const *exists;
    std::vector<Slice> slices;
    std::vector<Slot> slots;
    std::vector<size_t> foff, eoff;
    const Slot *dslots = nullptr;
    const uint8_t *dbits = nullptr;
    const uint8_t *dextra = nullptr;  // stage()'s extra bytes on the device
    int64_t *list_ids = nullptr;      // [nparts][nq][k]
    float *list_dist = nullptr;
    CallIO::Out out{};
    int32_t *dpart = nullptr;

    int nparts() const { return (int)rows.size(); }

    // The fused parts in group order, a new slice whenever the next part's
    // cost(p) would take the slice's sum past `limit`.  open(p, e, cur) sets
    // slot e of part p from the slice's running sums and advances them;
    // seal(e, cur) sets the sentinel from the slice's totals.
    template <typename Cost, typename Open, typename Seal>
    void build_slices(const std::vector<char> &fused, int64_t limit, Cost &&cost, Open &&open, Seal &&seal) {
        Slice cur{};
        int64_t used = 0;
        auto close = [&] {
            if (cur.nslots == 0) return;
            Slot end{};
            seal(end, cur);
            end.part = -1;
            slots.push_back(end);
            slices.push_back(cur);
            cur = Slice{};
            cur.first_slot = (int)slots.size();
            used = 0;
        };
        for (int p = 0; p < nparts(); ++p) {
            if (!fused[p]) continue;
            const int64_t c = cost(p);
            if (cur.nslots > 0 && used + c > limit) close();
            Slot e{};
            e.part = p;
            open(p, e, cur);
            slots.push_back(e);
            cur.nslots += 1;
            used += c;
        }
        close();
    }

    // this call's bitmaps of part p on the device
    const uint8_t *part_filter(int p) const {
        return !(filters && filters[p]) ? nullptr : dev ? filters[p] : dbits + foff[p];
    }
    const uint8_t *part_exists(int p) const {
        return !(exists && exists[p]) ? nullptr : dev ? exists[p] : dbits + eoff[p];
    }

    // the slot tables, the host bitmaps of every part and `extra` (host bytes
    // of the call, or null) through one pinned buffer, one copy to the device
    void stage(const void *extra, size_t extra_bytes) {
        const int np = nparts();
        foff.assign(np, (size_t)-1);
        eoff.assign(np, (size_t)-1);
        size_t bits_bytes = 0;
        if (!dev)
            for (int p = 0; p < np; ++p) {
                if (filters && filters[p]) foff[p] = bitmap_slot(bits_bytes, rows[p]);
                if (exists && exists[p]) eoff[p] = bitmap_slot(bits_bytes, rows[p]);
            }
        const size_t slot_bytes = (size_t)round_up((int64_t)(sizeof(Slot) * slots.size()), 16);
        const size_t total = slot_bytes + bits_bytes + (size_t)round_up((int64_t)extra_bytes, 16);
        if (total == 0) return;
        auto *pin = (unsigned char *)ws.pg_pin_in.get(total);
        auto *dbuf = (unsigned char *)ws.pg_slots.get(total);
        dslots = (const Slot *)dbuf;
        dbits = dbuf + slot_bytes;
        dextra = dbuf + slot_bytes + bits_bytes;
        for (int p = 0; p < np && !dev; ++p) {
            const size_t bm = (size_t)((rows[p] + 7) / 8);
            if (foff[p] != (size_t)-1) std::memcpy(pin + slot_bytes + foff[p], filters[p], bm);
            if (eoff[p] != (size_t)-1) std::memcpy(pin + slot_bytes + eoff[p], exists[p], bm);
        }
        if (extra_bytes) std::memcpy(pin + slot_bytes + bits_bytes, extra, extra_bytes);
        for (Slot &e : slots) {
            if (e.part < 0) continue;
            e.filter = part_filter(e.part);
            e.exists = part_exists(e.part);
        }
        if (!slots.empty()) std::memcpy(pin, slots.data(), sizeof(Slot) * slots.size());
        MQVS_HIP(hipMemcpyAsync(dbuf, pin, total, hipMemcpyHostToDevice, s));
    }

    // per-part lists [nparts][nq][k] and the outputs
    void lists_and_outputs(int32_t *out_part, int64_t *out_ids, float *out_dist) {
        const size_t nlist = (size_t)nparts() * nq * k, nout = (size_t)nq * k;
        auto *lbuf = (unsigned char *)ws.pg_lists.get(nlist * 12 + 16);
        list_ids = (int64_t *)lbuf;
        list_dist = (float *)(lbuf + nlist * 8);
        out = ws.io.out(nout, dev, out_ids, out_dist);
        dpart = dev ? out_part : (int32_t *)ws.pg_part.get(sizeof(int32_t) * nout);
    }
    int64_t *part_ids(int p) const { return list_ids + (size_t)p * nq * k; }
    float *part_dist(int p) const { return list_dist + (size_t)p * nq * k; }

    // the merge (order: the metric whose key orders the lists; launches += 1),
    // and the call's one wait.  words (optional): nwords bytes of the device the
    // call also wants on the host (hwords) after that wait.
    void merge_and_wait(int order, int32_t *out_part, int32_t &launches, const void *words = nullptr,
                        void *hwords = nullptr, size_t nwords = 0) {
        const int np = nparts();
        const size_t nout = (size_t)nq * k;
        uint4 *scratch =
            (int64_t)np * k > kSortCap ? (uint4 *)ws.pg_sort.get(sizeof(uint4) * 2 * (size_t)np * k * nq) : nullptr;
        launch_merge_shards(np, nq, k, order, list_ids, list_dist, out.ids, out.dist, true, scratch, s, dpart);
        MQVS_HIP(hipGetLastError());
        launches += 1;
        ws.io.finish_begin(out, s);
        const size_t part_bytes = dev ? 0 : (size_t)round_up((int64_t)(sizeof(int32_t) * nout), 16);
        unsigned char *pin = part_bytes + nwords ? (unsigned char *)ws.pg_pin_out.get(part_bytes + nwords) : nullptr;
        if (part_bytes) MQVS_HIP(hipMemcpyAsync(pin, dpart, sizeof(int32_t) * nout, hipMemcpyDeviceToHost, s));
        if (nwords) MQVS_HIP(hipMemcpyAsync(pin + part_bytes, words, nwords, hipMemcpyDeviceToHost, s));
        host_wait(s);
        ws.io.finish_end(out);
        if (part_bytes) std::memcpy(out_part, pin, sizeof(int32_t) * nout);
        if (nwords) std::memcpy(hwords, pin + part_bytes, nwords);
    }
};

}  // namespace mqvs
