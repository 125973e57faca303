// Compile-and-run check of the binary index-group part of
// include/mqvs_vector_index.hpp (BinaryIndexGroup over BinaryGpuIndexes):
//   shim_index_group_binary errors          no GPU needed: the argument checks' error mappings
//   shim_index_group_binary gpu IN OUT      the case of file IN (written by
//       tests/test_shim_index_group_binary.py, which holds the reference) searched
//       through BinaryIndexGroup::search; the labelled rows go to file OUT
// IN:  int32 nparts, nbytes, nq, k, params length; the search params; per
//      part: int64 n, row_offset, nlist, n * nbytes code bytes, then twice
//      (filter, row_exists) a flag byte and, when it is 1, (n + 7) / 8 bitmap
//      bytes; nq * nbytes query bytes
// OUT: int64 rows; per row uint32 part, label, vector_id and the float distance
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mqvs_vector_index.hpp"

namespace MI = VectorIndex::MI355X;

template <typename F>
static bool throws(int code, const F &f) {
    try {
        f();
    } catch (const DB::Exception &e) {
        if (e.code() == code) return true;
        std::printf("code %d, want %d: %s\n", e.code(), code, e.what());
        return false;
    }
    std::printf("no exception, want code %d\n", code);
    return false;
}

static int errors() {
    uint8_t q[4] = {0};
    int32_t part[4];
    int64_t ids[4];
    float dist[4];
    // (every one of these fails before any device work)
    bool ok = throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] {
        MI::check(mqvs_index_group_search_binary(nullptr, q, 1, 1, "", nullptr, nullptr, part, ids, dist, 0, nullptr));
    });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS,
                      [&] { MI::BinaryIndexGroup empty(std::vector<const MI::BinaryGpuIndex *>{}); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS,
                      [&] { MI::BinaryIndexGroup null_index(std::vector<const MI::BinaryGpuIndex *>{nullptr}); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_index_group_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)); });
    if (!ok) return 1;
    std::printf("errors ok\n");
    return 0;
}

static bool read_all(std::FILE *f, void *dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }

static int gpu(const char *in_path, const char *out_path) {
    std::FILE *f = std::fopen(in_path, "rb");
    if (!f) return 2;
    int32_t head[5];
    if (!read_all(f, head, sizeof(head))) return 2;
    const int np = head[0], nbytes = head[1], nq = head[2], k = head[3];
    std::string params((size_t)head[4], '\0');
    if (!read_all(f, &params[0], params.size())) return 2;
    std::vector<std::vector<uint8_t>> codes(np), flt(np), ex(np);
    std::vector<MI::BinaryPartScan> parts;
    std::vector<MI::BinaryGpuIndex> indexes;
    parts.reserve(np);
    indexes.reserve(np);
    for (int p = 0; p < np; ++p) {
        int64_t nr[3];
        if (!read_all(f, nr, sizeof(nr))) return 2;
        codes[p].resize((size_t)nr[0] * nbytes);
        if (!read_all(f, codes[p].data(), codes[p].size())) return 2;
        for (std::vector<uint8_t> *bm : {&flt[p], &ex[p]}) {
            uint8_t has = 0;
            if (!read_all(f, &has, 1)) return 2;
            if (has) {
                bm->resize((size_t)(nr[0] + 7) / 8);
                if (!read_all(f, bm->data(), bm->size())) return 2;
            }
        }
        parts.emplace_back(codes[p].data(), nr[0], nbytes, MQVS_METRIC_HAMMING, 256, nr[1]);
        indexes.emplace_back(parts[p], "BINARYMSTG", "nlist=" + std::to_string(nr[2]) + ",kmeans_iters=8");
    }
    std::vector<uint8_t> q((size_t)nq * nbytes);
    if (!read_all(f, q.data(), q.size())) return 2;
    std::fclose(f);

    std::vector<const MI::BinaryGpuIndex *> ptrs;
    std::vector<const uint8_t *> filters, exists;
    for (int p = 0; p < np; ++p) {
        ptrs.push_back(&indexes[p]);
        filters.push_back(flt[p].empty() ? nullptr : flt[p].data());
        exists.push_back(ex[p].empty() ? nullptr : ex[p].data());
    }
    MI::BinaryIndexGroup group(ptrs);
    const MI::PartRows pr = group.search(q.data(), nq, nbytes, k, params, filters.data(), exists.data());
    const mqvs_index_group_stats st = MI::BinaryIndexGroup::lastStats();
    std::printf("fused %d\n", st.parts == np && st.fused_parts == np && st.looped_parts == 0 ? 1 : 0);

    std::FILE *o = std::fopen(out_path, "wb");
    if (!o) return 2;
    const int64_t rows = (int64_t)pr.label.size();
    std::fwrite(&rows, sizeof(rows), 1, o);
    for (int64_t i = 0; i < rows; ++i) {
        const uint32_t rec[3] = {pr.part[i], pr.label[i], pr.vector_id[i]};
        std::fwrite(rec, sizeof(rec), 1, o);
        std::fwrite(&pr.distance[i], sizeof(float), 1, o);
    }
    std::fclose(o);

    const bool width = throws(DB::ErrorCodes::LOGICAL_ERROR,
                              [&] { (void)group.search(q.data(), nq, nbytes + 1, k, params); });
    std::printf("bad width %d\n", width ? 1 : 0);
    const bool key = throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { (void)group.search(q.data(), nq, nbytes, k, "beam=3"); });
    std::printf("bad key %d\n", key ? 1 : 0);
    // the fallback callable runs instead when the device fails
    std::vector<int32_t> gp((size_t)nq * k);
    std::vector<int64_t> gi(gp.size());
    std::vector<float> gd(gp.size());
    int called = 0;
    MI::check(mqvs_inject_fault(MQVS_ERR_DEVICE, 1));
    group.search(q.data(), nq, k, params, nullptr, nullptr, gp.data(), gi.data(), gd.data(), 0,
                 [&](const uint8_t *, int32_t, int32_t, const std::string &, const uint8_t *const *,
                     const uint8_t *const *, int32_t *, int64_t *, float *) { ++called; });
    std::printf("fallback %d\n", called == 1 ? 1 : 0);
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && std::string(argv[1]) == "errors") return errors();
        if (argc >= 4 && std::string(argv[1]) == "gpu") return gpu(argv[2], argv[3]);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::fprintf(stderr, "usage: shim_index_group_binary errors | gpu IN OUT\n");
    return 2;
}
