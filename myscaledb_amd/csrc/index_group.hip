// index_group.hip -- many binary indexed parts searched in one fused call
// (mqvs_index_group_*, include/mqvs.h).
//
// The fused route is mqvs_index_search_binary's chain with a batch dimension
// over the parts (the slots of BivfGroupSlot, index_kernels.h):
//   1. query codes       uploaded and zero padded once per call
//   2. grouped coarse    k_bivf_group_cdist: k_bivf_cdist's 256-centroid tiles
//                        of every (ranked slot, query); k_bivf_group_pick: per
//                        (slot, query) k_bivf_pick's rule, or every list in
//                        order for a slot that probes all of its lists
//   3. grouped scan      k_bivf_group_scan: k_bivf_scan's work items of every
//                        slot; records to the (slot, query) regions
//   4. grouped select    k_bivf_group_select: k_final_select's body per (slot,
//                        query) -> per-part top-k lists
//   (2 - 4 once per slice of parts whose records and centroid distances fit
//   the scratch budget)
//   5. id map            k_bivf_group_map, when a fused part has a row-ids map
//   6. stats             k_bivf_group_stats: the per-part stats words, summed
//   7. merge             k_merge_shards (part merge) with the list index out
// Parts the fused route does not take run search_binary_index_impl on the same
// stream, with their resolved nprobe, into their list of the same merge.
// Nothing here depends on what a kernel found: a record region holds every
// position of its probed lists, and the call has one host wait, after the
// merge.
//
// The group borrows its indexes and reads them at every search (lists, row-ids
// map, the segment's row offset): it holds no device memory of its own.
//
// What the call saves is the per-part fixed cost of the loop it replaces.
// Measured with 256-bit codes, k 100, default nlist and nprobe
// (profiles/index_group): the DEVICE_PTRS | ASYNC loop of
// mqvs_index_search_binary calls plus the merge costs 100 - 150 us per part at
// nq 1 and 200 - 260 us at nq 16 and 128 more than this call (17.3 ms against
// 0.54 ms for 128 parts of 65536 rows at nq 1); the synchronous loop another
// 40 - 110 us per part.  The fused route won every measured case (8 x 1048576,
// 32 x 262144 and 128 x 65536 rows; nq 1, 16, 128; both metrics), so it has no
// row limit.
#include <hip/hip_runtime.h>

#include <vector>

#include "group_call.h"
#include "index_internal.h"

struct mqvs_index_group {
    std::vector<mqvs_index *> idx;
    int device = 0;
    int dim_bits = 0;
    int code_bytes = 0, code_words = 0;
};

namespace mqvs {

static thread_local mqvs_index_group_stats t_igroup_stats{};

static mqvs_index_group *igroup_create(const mqvs_index_t *indexes, int nparts) {
    if (nparts < 1 || !indexes) fail(MQVS_ERR_BAD_ARGUMENTS, "an index group needs at least one index");
    for (int p = 0; p < nparts; ++p)
        if (!indexes[p]) fail(MQVS_ERR_BAD_ARGUMENTS, "null index in an index group");
    for (int p = 0; p < nparts; ++p) {
        const mqvs_index *ix = indexes[p];
        if (!ix->binary)
            fail(MQVS_ERR_NOT_IMPLEMENTED, "float index groups are not built: an index group takes binary "
                                           "(BINARYMSTG) indexes only");
        if (ix->seg->device != indexes[0]->seg->device)
            fail(MQVS_ERR_BAD_ARGUMENTS, "indexes of an index group are on different devices");
    }
    for (int p = 0; p < nparts; ++p)
        if (indexes[p]->seg->d != indexes[0]->seg->d)
            fail(MQVS_ERR_LOGICAL, "indexes of an index group differ in dim_bits");
    auto *g = new mqvs_index_group();
    g->idx.assign(indexes, indexes + nparts);
    const mqvs_segment *s0 = indexes[0]->seg;
    g->device = s0->device;
    g->dim_bits = s0->d;
    g->code_bytes = s0->code_bytes;
    g->code_words = s0->code_words;
    return g;
}

// slots [first_slot, first_slot + nslots) (+ the sentinel) of one grouped
// coarse + scan + select, with the running sums of the slots' prefix fields
struct IndexSlice {
    int first_slot, nslots;
    int64_t cents, ctiles, items, cands;
};
using IndexGroupCall = GroupCall<BivfGroupSlot, IndexSlice>;

static void igroup_search_binary(mqvs_index_group *g, const uint8_t *queries, int nq, int k, const char *params,
                                 const uint8_t *const *filters, const uint8_t *const *exists, int32_t *out_part,
                                 int64_t *out_ids, float *out_dist, uint32_t flags, hipStream_t user_stream) {
    check_group_args(g, "index group", nullptr, nq, k, queries, out_part, out_ids, out_dist);
    const int nparts = (int)g->idx.size();

    // ---- the search parameters: one metric; nprobe per part
    const auto pm = parse_params(params);
    check_keys(pm, {"alpha", "nprobe", "num_reorder", "metric"}, "search");
    const int metric = pm.count("metric") ? binary_metric_of(pm.at("metric"), "metric") : g->idx[0]->metric;
    // (accepted and ignored: the scan is exact, nothing is re-ordered)
    (void)num_param(pm, "num_reorder", 1, 1, (double)kLargeCap);
    // an explicit nprobe is cut to each part's list count (parts of one table
    // differ in it); without one each part resolves its own from alpha
    const bool explicit_np = pm.count("nprobe") != 0;
    const int want_np = explicit_np ? (int)num_param(pm, "nprobe", 1, 1, (double)kSortCap) : 0;
    std::vector<int> nprobe(nparts);
    for (int p = 0; p < nparts; ++p)
        nprobe[p] =
            explicit_np ? (int)std::min<int64_t>(want_np, g->idx[p]->nlist) : search_nprobe(g->idx[p], pm);
    mqvs_index_group_stats st;
    if (!group_begin(nparts, nq, k, st, t_igroup_stats)) return;
    GroupScope sc(g->device, flags, user_stream);
    Workspace &ws = sc.ws;
    hipStream_t s = sc.s;
    const bool dev = flags & MQVS_F_DEVICE_PTRS;
    constexpr int kOrder = MQVS_METRIC_L2;  // ascending finite values: ord_asc key, (key, row) ties
    const int cw = g->code_words;

    // ---- the routes: a part is fused when its own scratch (every query's
    // records and centroid distances) fits the scratch budget
    const int64_t budget = (int64_t)scratch_budget();
    std::vector<char> fused(nparts, 0);
    std::vector<int64_t> rows(nparts);
    int nfused = 0;
    bool any_map = false;
    for (int p = 0; p < nparts; ++p) {
        const mqvs_index *ix = g->idx[p];
        rows[p] = ix->seg->n;
        const int64_t cap = binary_index_cap(ix, nprobe[p]);
        fused[p] = k <= kSortCap && cap <= INT32_MAX && (int64_t)nq * binary_index_scratch(ix, nprobe[p]) <= budget;
        nfused += fused[p];
        any_map = any_map || (fused[p] && ix->row_ids_map);
    }
    st.fused_parts = nfused;
    st.looped_parts = nparts - nfused;

    // ---- inputs.  The host queries ride with the slot tables and bitmaps
    IndexGroupCall c{rows, ws, s, dev, nq, k, filters, exists};
    int64_t nprobes = 0, ncounts = 0;  // of the whole call
    c.build_slices(
        fused, budget, [&](int p) { return (int64_t)nq * binary_index_scratch(g->idx[p], nprobe[p]); },
        [&](int p, BivfGroupSlot &e, IndexSlice &cur) {
            const mqvs_index *ix = g->idx[p];
            const bool rank = nprobe[p] < ix->nlist;
            e.bcent = ix->bcent;
            e.bplane = ix->bplane;
            e.perm = ix->perm;
            e.list_off = ix->list_off;
            e.row_ids_map = ix->row_ids_map;
            e.row_offset = ix->seg->row_offset;
            e.nlist = (int32_t)ix->nlist;
            e.nprobe = nprobe[p];
            e.nch = (int32_t)((ix->max_list + 255) / 256);
            e.cap = (int32_t)binary_index_cap(ix, nprobe[p]);
            e.cent0 = cur.cents;
            e.ctile0 = cur.ctiles;
            e.item0 = cur.items;
            e.cand0 = cur.cands;
            e.probe0 = nprobes;
            e.count0 = ncounts;
            if (rank) {
                cur.cents += ix->nlist;
                cur.ctiles += (int64_t)nq * ((ix->nlist + 255) / 256);
            }
            cur.items += (int64_t)nq * e.nprobe * e.nch;
            cur.cands += (int64_t)nq * e.cap;
            nprobes += (int64_t)nq * e.nprobe;
            ncounts += nq;
        },
        [](BivfGroupSlot &end, const IndexSlice &cur) {
            end.cent0 = cur.cents;
            end.ctile0 = cur.ctiles;
            end.item0 = cur.items;
            end.cand0 = cur.cands;
        });
    c.stage(dev ? nullptr : queries, dev ? 0 : (size_t)nq * g->code_bytes);
    const uint8_t *dq = dev ? queries : c.dextra;  // [nq][code_bytes] on the device
    c.lists_and_outputs(out_part, out_ids, out_dist);

    // ---- the fused route
    // [overflow 4][unused 4][stats: values, items, plane bytes, pairs]
    int *fl = nullptr;
    if (nfused > 0) {
        fl = (int *)ws.pg_q.get(sizeof(int) * 16);
        launch_fill2((uint32_t *)fl, 16, 0u, nullptr, 0, 0u, s);
        MQVS_HIP(hipGetLastError());
        st.launches += 1;
        int64_t *dstats = (int64_t *)(fl + 8);
        // the query codes, zero padded to the segments' row stride, once per call
        uint32_t *qc = (uint32_t *)ws.pg_qvars.get((size_t)nq * cw * 4);
        upload_codes(qc, cw, dq, g->code_bytes, nq, true, s);
        int64_t max_cents = 0, max_cands = 0;
        for (const IndexSlice &sl : c.slices) {
            max_cents = std::max(max_cents, sl.cents);
            max_cands = std::max(max_cands, sl.cands);
        }
        // the slices' scratch: records and centroid distances; the call's probes and counters
        Cand *cand = (Cand *)ws.pg_matrix.get(sizeof(Cand) * (size_t)std::max<int64_t>(max_cands, 1));
        uint32_t *cdist = (uint32_t *)ws.pg_cdist.get(sizeof(uint32_t) * (size_t)nq * std::max<int64_t>(max_cents, 1));
        auto *pbuf = (unsigned char *)ws.pg_probes.get(sizeof(int64_t) * (size_t)nprobes + sizeof(int) * (size_t)ncounts);
        int64_t *probes = (int64_t *)pbuf;
        int *count = (int *)(pbuf + sizeof(int64_t) * (size_t)nprobes);
        BivfParams base{};
        base.code_words = cw;
        base.nbits = g->dim_bits;
        base.nq = nq;
        base.qcodes = qc;
        base.probes = probes;
        base.cand = cand;
        for (const IndexSlice &sl : c.slices) {
            const BivfGroupSlot *ds = c.dslots + sl.first_slot;
            launch_bivf_group_coarse(ds, sl.nslots, sl.ctiles, cw, qc, nq, cdist, sl.cents, probes, count, s);
            MQVS_HIP(hipGetLastError());
            st.launches += sl.ctiles > 0 ? 2 : 1;
            if (sl.items > 0) {
                launch_bivf_group_scan(base, ds, sl.nslots, sl.items, count, metric, s);
                MQVS_HIP(hipGetLastError());
                st.launches += 1;
            }
            launch_bivf_group_select(cand, count, ds, sl.nslots, nq, k, c.list_ids, c.list_dist, fl, s);
            MQVS_HIP(hipGetLastError());
            st.launches += 1;
        }
        const int nentries = (int)c.slots.size();
        if (any_map) {
            // decoupled parts: results in the new part's row ids
            launch_bivf_group_map(c.dslots, nentries, (int64_t)nq * k, c.list_ids, s);
            MQVS_HIP(hipGetLastError());
            st.launches += 1;
        }
        launch_bivf_group_stats(c.dslots, nentries, nq, cw, probes, count, dstats, s);
        MQVS_HIP(hipGetLastError());
        st.launches += 1;
    }

    // ---- the per-part route (each search ends in its own host wait)
    for (int p = 0; p < nparts; ++p) {
        if (fused[p]) continue;
        search_binary_index_impl(g->idx[p], dq, nq, k, metric, nprobe[p], c.part_filter(p), c.part_exists(p),
                                 c.part_ids(p), c.part_dist(p),
                                 (flags & ~(uint32_t)MQVS_F_ASYNC) | (uint32_t)MQVS_F_DEVICE_PTRS, s, nullptr);
    }

    // ---- the merge, and the call's one wait
    int64_t words[8] = {};  // fl's 16 words: the overflow word first, the four stats sums in words[4, 8)
    if (nfused > 0)
        c.merge_and_wait(kOrder, out_part, st.launches, fl, words, sizeof(words));
    else
        c.merge_and_wait(kOrder, out_part, st.launches);
    if ((int32_t)(words[0] & 0xFFFFFFFF)) fail(MQVS_ERR_DEVICE, "index group search: a record region overflowed");
    st.values = words[4];
    st.items = words[5];
    st.plane_bytes = words[6];
    st.pairs = words[7];
    st.total_ms = sc.total_ms();
    t_igroup_stats = st;
}

}  // namespace mqvs

using namespace mqvs;

extern "C" {

int mqvs_index_group_create(const mqvs_index_t *indexes, int32_t nparts, mqvs_index_group_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        *out = igroup_create(indexes, nparts);
    });
}

int mqvs_index_group_free(mqvs_index_group_t group) {
    return guarded([&] { delete group; });
}

int mqvs_index_group_info(mqvs_index_group_t group, int32_t *nparts, int64_t *rows, int32_t *dim_bits, int64_t *lists,
                          size_t *hbm_bytes) {
    return guarded([&] {
        if (!group) fail(MQVS_ERR_BAD_ARGUMENTS, "null index group");
        int64_t r = 0, l = 0;
        for (const mqvs_index *ix : group->idx) {
            r += ix->seg->n;
            l += ix->nlist;
        }
        if (nparts) *nparts = (int32_t)group->idx.size();
        if (rows) *rows = r;
        if (dim_bits) *dim_bits = group->dim_bits;
        if (lists) *lists = l;
        if (hbm_bytes) *hbm_bytes = 0;
    });
}

int mqvs_index_group_search_binary(mqvs_index_group_t group, const uint8_t *queries, int32_t nq, int32_t k,
                                   const char *params, const uint8_t *const *filters,
                                   const uint8_t *const *row_exists, int32_t *out_part, int64_t *out_ids,
                                   float *out_dist, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{11, (uint64_t)(uintptr_t)group, (uint64_t)nq, (uint64_t)k, wait_str_hash(params),
                      filters != nullptr, row_exists != nullptr, flags};
        igroup_search_binary(group, queries, nq, k, params, filters, row_exists, out_part, out_ids, out_dist, flags,
                             (hipStream_t)stream);
    });
}

int mqvs_index_group_last_stats(mqvs_index_group_stats *out) {
    if (!out) return MQVS_ERR_BAD_ARGUMENTS;
    *out = t_igroup_stats;
    return MQVS_OK;
}

}  // extern "C"
