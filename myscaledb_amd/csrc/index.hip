// index.hip -- the index path of libmqvs: an MSTG-type vector index over a
// resident segment (mqvs_index_*; C-ABI in include/mqvs.h).
//
// Reference seam (src/VectorIndex/Common/VIWithDataPart.cpp):
//   createIndex -> Search::createVectorIndex<..., FloatVector>(...)   :416-447
//   VIWithColumnInPart::search -> VectorIndex::search(queries, k, params,
//       first_stage_only, filter ∩ delete bitmap)                    :858-957
//   computeTopDistanceSubset (two-stage search, stage 2)              :838-856
// The MSTG library itself is absent from the snapshot, so the
// index is this library's own design for HBM and MFMA:
//   build                     index_build.hip (float: k-means lists as a bf16
//                             or fp8 plane; binary: k-majority lists; the list
//                             count's auto-tuning)
//   search of a float index   index_search.hip
//   search of a binary index  index_search_binary.hip
//   save / load               index_blob.hip
// This file holds what they all use -- the thread's index workspace, the
// parameter parser, nprobe_of, free_index -- the C glue of every index entry
// point, and mqvs_decoupled_filter; index_internal.h what the files share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "index_internal.h"

namespace mqvs {
mqvs_segment *index_segment(mqvs_index *idx) { return idx ? idx->seg : nullptr; }
}  // namespace mqvs

namespace mqvs {

thread_local mqvs_index_search_stats g_istats{};

static thread_local std::map<int, IndexWorkspace> *g_iws = nullptr;

// mqvs_thread_release: the calling thread's index workspaces (scratch,
// events, side stream, pinned words)
void index_thread_release() {
    if (!g_iws) return;
    for (auto &kv : *g_iws) {
        (void)hipSetDevice(kv.first);
        ws_detach_ext(kv.first, &kv.second);
        kv.second.release();
    }
    g_iws->clear();
}

IndexWorkspace &index_workspace(int device) {
    if (!g_iws) g_iws = new std::map<int, IndexWorkspace>();  // leaked at exit on purpose
    IndexWorkspace &w = (*g_iws)[device];
    w.init();
    return w;
}


// ---- Search::Parameters: "k=v,k=v" ----------------------------------------
std::map<std::string, std::string> parse_params(const char *s) {
    std::map<std::string, std::string> out;
    if (!s) return out;
    std::string str(s);
    size_t i = 0;
    while (i < str.size()) {
        size_t j = str.find(',', i);
        if (j == std::string::npos) j = str.size();
        std::string kv = str.substr(i, j - i);
        i = j + 1;
        auto trim = [](std::string x) {
            const auto b = x.find_first_not_of(" \t'\"");
            const auto e = x.find_last_not_of(" \t'\"");
            return b == std::string::npos ? std::string() : x.substr(b, e - b + 1);
        };
        kv = trim(kv);
        if (kv.empty()) continue;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) fail(MQVS_ERR_BAD_ARGUMENTS, "index parameter `" + kv + "` is not key=value");
        std::string key = trim(kv.substr(0, eq)), val = trim(kv.substr(eq + 1));
        for (auto &ch : key) ch = (char)std::tolower((unsigned char)ch);
        out[key] = val;
    }
    return out;
}

double num_param(const std::map<std::string, std::string> &m, const std::string &key, double dflt,
                        double lo, double hi) {
    auto it = m.find(key);
    if (it == m.end()) return dflt;
    char *end = nullptr;
    const double v = std::strtod(it->second.c_str(), &end);
    if (!end || *end != '\0' || it->second.empty() || !(v >= lo && v <= hi))
        fail(MQVS_ERR_BAD_ARGUMENTS, "index parameter `" + key + "` = `" + it->second + "` out of range [" +
                                         std::to_string(lo) + ", " + std::to_string(hi) + "]");
    return v;
}

void check_keys(const std::map<std::string, std::string> &m, const std::vector<std::string> &valid,
                       const char *what) {
    for (auto &kv : m) {
        if (std::find(valid.begin(), valid.end(), kv.first) == valid.end()) {
            std::string list;
            for (auto &v : valid) list += (list.empty() ? "" : ",") + v;
            fail(MQVS_ERR_BAD_ARGUMENTS, std::string("MSTG doesn't support ") + what + " parameter: `" + kv.first +
                                             "`, valid parameters is [" + list + "].");
        }
    }
}

// nprobe for a search alpha: nprobe(3) = base, doubling per unit of alpha;
// the base probes 1/256 of the lists and at least 4 lists and 4096 rows
int nprobe_of(const mqvs_index *ix, double alpha) {
    const double rows = (double)std::max<int64_t>(ix->rows_indexed, 1);
    // (an index whose list count was chosen from its data knows the nprobe
    // that reached recall@10 0.95 on the build's sample: alpha 3 probes 1.5x
    // that, a margin for queries unlike the part's own rows)
    const double base = ix->np95 > 0 ? (double)(ix->np95 + std::max(1, ix->np95 / 2))
                                     : std::max({4.0, std::ceil((double)ix->nlist / 256.0),
                                                 std::ceil(4096.0 * ix->nlist / rows)});
    const double np = std::ceil(base * std::pow(2.0, alpha - 3.0));
    return (int)std::max<double>(1.0, std::min<double>(np, (double)std::min<int64_t>(ix->nlist, kSortCap)));
}

void free_index(mqvs_index *ix) {
    if (!ix) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (ix->seg) (void)hipSetDevice(ix->seg->device);
    if (ix->cent) segment_release(ix->cent);
    for (void *q : {(void *)ix->plane, (void *)ix->perm, (void *)ix->pnorm, (void *)ix->list_off, (void *)ix->cplane,
                    (void *)ix->cperm, (void *)ix->cpnorm, (void *)ix->clist_off, (void *)ix->row_ids_map,
                    (void *)ix->yrec, (void *)ix->bplane, (void *)ix->bcent, (void *)ix->plane8,
                    (void *)ix->pscale})
        if (q) (void)hipFree(q);
    if (cur >= 0) (void)hipSetDevice(cur);
    delete ix;
}

}  // namespace mqvs

using namespace mqvs;

extern "C" {

int mqvs_index_build(mqvs_segment_t seg, const char *index_type, const char *params, mqvs_index_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        *out = build_impl(seg, index_type, params);
    });
}

int mqvs_index_free(mqvs_index_t idx) {
    return guarded([&] { free_index(idx); });
}

int mqvs_index_info(mqvs_index_t idx, mqvs_index_info_t *out) {
    return guarded([&] {
        if (!idx || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        out->nlist = idx->nlist;
        out->npos = idx->npos;
        out->max_list = idx->max_list;
        out->rows_indexed = idx->rows_indexed;
        out->metric = idx->metric;
        out->dim = idx->seg->d;
        out->hbm_bytes = idx->bytes;
        out->build_ms = idx->build_ms;
    });
}

int mqvs_index_plane(mqvs_index_t idx, int32_t *format, size_t *plane_bytes) {
    return guarded([&] {
        if (!idx) fail(MQVS_ERR_BAD_ARGUMENTS, "null index");
        if (idx->binary) fail(MQVS_ERR_LOGICAL, "binary index: it has no float list plane");
        const bool fp8 = idx->plane_fmt == MQVS_INDEX_PLANE_FP8;
        if (format) *format = idx->plane_fmt;
        if (plane_bytes)
            *plane_bytes = (size_t)idx->npos * (size_t)idx->dpad * (fp8 ? 1 : 2) +
                           (fp8 ? sizeof(int16_t) * (size_t)idx->npos : 0);
    });
}

int mqvs_index_search_ex(mqvs_index_t idx, const float *queries, int32_t nq, int32_t k, const char *params,
                         const uint8_t *filter, const uint8_t *row_exists, int64_t chunk_ord_base, int64_t *out_ids,
                         float *out_dist, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        if (chunk_ord_base > INT32_MAX) fail(MQVS_ERR_BAD_ARGUMENTS, "chunk_ord_base out of range");
        WaitScope wsc{4, (uint64_t)(uintptr_t)idx, (uint64_t)nq, (uint64_t)k, wait_str_hash(params), filter != nullptr,
                      row_exists != nullptr, flags};
        search_index_impl(idx, queries, nq, k, params, filter, row_exists, out_ids, out_dist, flags,
                          (hipStream_t)stream, 0, 0, chunk_ord_base);
    });
}

int mqvs_index_search(mqvs_index_t idx, const float *queries, int32_t nq, int32_t k, const char *params,
                      const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                      uint32_t flags, mqvs_stream_t stream) {
    return mqvs_index_search_ex(idx, queries, nq, k, params, filter, row_exists, -1, out_ids, out_dist, flags, stream);
}

int mqvs_index_centroids(mqvs_index_t idx, float *out, int64_t cap) {
    return guarded([&] {
        if (!idx || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (idx->binary) fail(MQVS_ERR_LOGICAL, "binary index: read its centroids with mqvs_index_centroids_binary");
        if (!idx->cent) fail(MQVS_ERR_LOGICAL, "index has no centroid table");
        const int64_t need = idx->cent->n * (int64_t)idx->cent->d;
        if (cap < need) fail(MQVS_ERR_BAD_ARGUMENTS, "output holds " + std::to_string(cap) + " floats, " +
                                                         std::to_string(need) + " needed");
        DeviceGuard guard(idx->cent->device);
        MQVS_HIP(hipMemcpy(out, idx->cent->rows, sizeof(float) * (size_t)need, hipMemcpyDeviceToHost));
    });
}

int mqvs_index_probes(mqvs_index_t idx, const float *queries, int32_t nq, const char *params, int64_t *out_probes) {
    return guarded([&] {
        if (!idx || (nq > 0 && (!queries || !out_probes))) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (nq < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "nq must be non-negative");
        if (nq == 0) return;
        WaitScope wsc{5, (uint64_t)(uintptr_t)idx, (uint64_t)nq, wait_str_hash(params)};
        // k 1: the coarse step does not depend on k; the search stops after it
        std::vector<int64_t> ids((size_t)nq);
        std::vector<float> dd((size_t)nq);
        search_index_impl(idx, queries, nq, 1, params, nullptr, nullptr, ids.data(), dd.data(), 0, nullptr, 0, 0, -1,
                          nullptr, out_probes);
    });
}

int mqvs_index_search_binary(mqvs_index_t idx, const uint8_t *queries, int32_t nq, int32_t k, const char *params,
                             const uint8_t *filter, const uint8_t *row_exists, int64_t *out_ids, float *out_dist,
                             uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        fault_point();
        WaitScope wsc{6, (uint64_t)(uintptr_t)idx, (uint64_t)nq, (uint64_t)k, wait_str_hash(params), filter != nullptr,
                      row_exists != nullptr, flags};
        search_binary_index_impl(idx, queries, nq, k, params, filter, row_exists, out_ids, out_dist, flags,
                                 (hipStream_t)stream, nullptr);
    });
}

int mqvs_index_centroids_binary(mqvs_index_t idx, uint8_t *out, int64_t cap_bytes) {
    return guarded([&] {
        if (!idx || !out) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (!idx->binary) fail(MQVS_ERR_LOGICAL, "Float32 index: read its centroids with mqvs_index_centroids");
        const int64_t nb = idx->seg->code_bytes;
        const int64_t need = idx->nlist * nb;
        if (cap_bytes < need) fail(MQVS_ERR_BAD_ARGUMENTS, "output holds " + std::to_string(cap_bytes) + " bytes, " +
                                                               std::to_string(need) + " needed");
        DeviceGuard guard(idx->seg->device);
        MQVS_HIP(hipMemcpy2D(out, (size_t)nb, idx->bcent, (size_t)idx->seg->code_words * 4, (size_t)nb,
                             (size_t)idx->nlist, hipMemcpyDeviceToHost));
    });
}

int mqvs_index_probes_binary(mqvs_index_t idx, const uint8_t *queries, int32_t nq, const char *params,
                             int64_t *out_probes) {
    return guarded([&] {
        if (!idx || (nq > 0 && (!queries || !out_probes))) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (nq < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "nq must be non-negative");
        if (nq == 0) return;
        WaitScope wsc{7, (uint64_t)(uintptr_t)idx, (uint64_t)nq, wait_str_hash(params)};
        // k 1: the coarse step does not depend on k; the search stops after it
        std::vector<int64_t> ids((size_t)nq);
        std::vector<float> dd((size_t)nq);
        search_binary_index_impl(idx, queries, nq, 1, params, nullptr, nullptr, ids.data(), dd.data(), 0, nullptr,
                                 out_probes);
    });
}

int mqvs_index_save_size(mqvs_index_t idx, size_t *bytes) {
    return guarded([&] {
        if (!idx || !bytes) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        *bytes = blob_bytes(idx);
    });
}

int mqvs_index_save(mqvs_index_t idx, uint8_t *out, size_t cap, size_t *written) {
    return guarded([&] {
        if (written) *written = 0;
        const size_t w = save_impl(idx, out, cap);
        if (written) *written = w;
    });
}

int mqvs_index_load(mqvs_segment_t seg, const uint8_t *blob, size_t bytes, mqvs_index_t *out) {
    return guarded([&] {
        if (!out) fail(MQVS_ERR_BAD_ARGUMENTS, "null output handle");
        *out = nullptr;
        *out = load_impl(seg, blob, bytes);
    });
}

int mqvs_index_blob_info(const uint8_t *blob, size_t bytes, mqvs_index_blob_info_t *out) {
    return guarded([&] { blob_info_impl(blob, bytes, out); });
}

int mqvs_index_lists(mqvs_index_t idx, int64_t *list_off, int64_t cap_off, int32_t *rows, int64_t cap_rows) {
    return guarded([&] {
        if (!idx || !list_off || (idx->npos > 0 && !rows)) fail(MQVS_ERR_BAD_ARGUMENTS, "null argument");
        if (cap_off < idx->nlist + 1 || cap_rows < idx->npos)
            fail(MQVS_ERR_BAD_ARGUMENTS, "outputs hold " + std::to_string(cap_off) + " offsets and " +
                                             std::to_string(cap_rows) + " rows, " + std::to_string(idx->nlist + 1) +
                                             " and " + std::to_string(idx->npos) + " needed");
        DeviceGuard guard(idx->seg->device);
        MQVS_HIP(hipMemcpy(list_off, idx->list_off, sizeof(int64_t) * (size_t)(idx->nlist + 1), hipMemcpyDeviceToHost));
        if (idx->npos > 0)
            MQVS_HIP(hipMemcpy(rows, idx->perm, sizeof(int32_t) * (size_t)idx->npos, hipMemcpyDeviceToHost));
    });
}

int mqvs_index_set_row_ids_map(mqvs_index_t idx, const uint64_t *row_ids_map, int64_t len, uint32_t flags) {
    return guarded([&] {
        if (!idx) fail(MQVS_ERR_BAD_ARGUMENTS, "null index");
        DeviceGuard guard(idx->seg->device);
        if (idx->row_ids_map) {
            MQVS_HIP(hipFree(idx->row_ids_map));
            idx->bytes -= sizeof(uint64_t) * (size_t)idx->row_ids_len;
            idx->row_ids_map = nullptr;
            idx->row_ids_len = 0;
        }
        if (!row_ids_map || len <= 0) return;
        if (len < idx->seg->row_offset + idx->seg->n)
            fail(MQVS_ERR_BAD_ARGUMENTS, "row_ids_map shorter than the indexed part (" + std::to_string(len) + " < " +
                                             std::to_string(idx->seg->row_offset + idx->seg->n) + ")");
        uint64_t *m = nullptr;
        if (hipMalloc((void **)&m, sizeof(uint64_t) * (size_t)len) != hipSuccess) {
            (void)hipGetLastError();
            fail(MQVS_ERR_MEMORY_LIMIT, "HBM allocation of the row id map failed");
        }
        MQVS_HIP(hipMemcpy(m, row_ids_map, sizeof(uint64_t) * (size_t)len,
                           (flags & MQVS_F_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        idx->row_ids_map = m;
        idx->row_ids_len = len;
        idx->bytes += sizeof(uint64_t) * (size_t)len;
    });
}

int mqvs_decoupled_filter(const uint8_t *new_filter, int64_t new_rows, const uint64_t *inverted_row_ids_map,
                          const uint8_t *inverted_row_sources_map, int64_t inverted_len, uint32_t own_id,
                          uint8_t *old_filter, int64_t old_rows, uint32_t flags, mqvs_stream_t stream) {
    return guarded([&] {
        if (new_rows < 0 || old_rows < 0 || inverted_len < 0) fail(MQVS_ERR_BAD_ARGUMENTS, "bad sizes");
        if ((new_rows && !new_filter) || (old_rows && !old_filter))
            fail(MQVS_ERR_BAD_ARGUMENTS, "null bitmap");
        if (inverted_len > 0 && (!inverted_row_ids_map || !inverted_row_sources_map))
            fail(MQVS_ERR_BAD_ARGUMENTS, "null inverted map");
        int dev = 0;
        MQVS_HIP(hipGetDevice(&dev));
        IndexWorkspace &ws = index_workspace(dev);
        WsScope scope(dev, &ws);
        hipStream_t s = stream ? (hipStream_t)stream : thread_stream(dev);
        scope.set_stream(s);
        const bool devp = flags & MQVS_F_DEVICE_PTRS;
        const int64_t nb = (new_rows + 7) / 8, ob = (old_rows + 7) / 8;
        const uint8_t *df = new_filter;
        const uint64_t *dinv = inverted_row_ids_map;
        const uint8_t *dsrc = inverted_row_sources_map;
        if (!devp) {
            auto *b = (uint8_t *)ws.dmap.get((size_t)nb + 16 + (size_t)inverted_len * 9 + 16);
            MQVS_HIP(hipMemcpyAsync(b, new_filter, nb, hipMemcpyHostToDevice, s));
            df = b;
            auto *inv = (uint64_t *)(b + (nb + 15) / 16 * 16);
            if (inverted_len) {
                MQVS_HIP(hipMemcpyAsync(inv, inverted_row_ids_map, 8 * (size_t)inverted_len, hipMemcpyHostToDevice, s));
                MQVS_HIP(hipMemcpyAsync((uint8_t *)(inv + inverted_len), inverted_row_sources_map, inverted_len,
                                        hipMemcpyHostToDevice, s));
            }
            dinv = inv;
            dsrc = (const uint8_t *)(inv + inverted_len);
        }
        auto *words = (uint32_t *)ws.dwords.get(4 * (size_t)((old_rows + 31) / 32) + 16);
        launch_decoupled_filter(df, new_rows, inverted_len ? dinv : nullptr, dsrc, inverted_len, own_id, words,
                                old_rows, s);
        MQVS_HIP(hipGetLastError());
        MQVS_HIP(hipMemcpyAsync(old_filter, words, ob, devp ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        if (!(devp && (flags & MQVS_F_ASYNC))) host_wait(s);
    });
}

int mqvs_index_last_stats(mqvs_index_search_stats *out) {
    if (!out) return MQVS_ERR_BAD_ARGUMENTS;
    *out = g_istats;
    return MQVS_OK;
}

}  // extern "C"
