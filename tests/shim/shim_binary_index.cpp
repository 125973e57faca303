// Compile-and-run check of the binary index part of include/mqvs_vector_index.hpp
// (BinaryPartScan / BinaryGpuIndex):
//   shim_binary_index errors   no GPU needed: the new seams' error mappings
//   shim_binary_index gpu      exhaustive index search == part search on a
//                              deterministic 3000 x 16-B table, the fallback
//                              hook under mqvs_inject_fault, setRowIdsMap
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
    const uint8_t codes[32] = {0};
    // a float metric on a binary column: NOT_IMPLEMENTED before any device work
    bool ok = throws(DB::ErrorCodes::NOT_IMPLEMENTED, [&] { MI::BinaryPartScan p(codes, 2, 16, MQVS_METRIC_L2, 8192); });
    // the C ABI's argument checks come before any device work too
    int64_t id[1];
    float dist[1];
    uint8_t cent[16];
    mqvs_index_t h = nullptr;
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] {
             MI::check(mqvs_index_search_binary(nullptr, codes, 1, 1, "", nullptr, nullptr, id, dist, 0, nullptr));
         });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_index_centroids_binary(nullptr, cent, 16)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS,
                      [&] { MI::check(mqvs_index_probes_binary(nullptr, codes, 1, "", id)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_index_build(nullptr, "BINARYMSTG", "", &h)); });
    if (!ok) return 1;
    std::printf("errors ok\n");
    return 0;
}

static int gpu() {
    const int n = 3000, nb = 16, nq = 4, k = 25;
    std::vector<uint8_t> codes((size_t)n * nb), q((size_t)nq * nb);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < nb; ++j) codes[(size_t)i * nb + j] = (uint8_t)((i * 131 + j * 29 + (i >> 3) * 7) % 251);
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < nb; ++j) q[(size_t)i * nb + j] = (uint8_t)(codes[(size_t)(i * 700 + 5) * nb + j] ^ (1u << (j & 7)));
    MI::BinaryPartScan part(codes.data(), n, nb, MQVS_METRIC_HAMMING, 512);
    MI::BinaryGpuIndex index(part, "BINARYMSTG", "nlist=12");
    std::vector<int64_t> a((size_t)nq * k), b((size_t)nq * k);
    std::vector<float> da((size_t)nq * k), db((size_t)nq * k);
    bool all = true;
    for (int metric : {MQVS_METRIC_HAMMING, MQVS_METRIC_JACCARD}) {
        part.search(q.data(), nq, nb, k, metric, nullptr, nullptr, a.data(), da.data());
        const std::string params = std::string("nprobe=12,metric=") + (metric == MQVS_METRIC_HAMMING ? "Hamming" : "Jaccard");
        index.search(q.data(), nq, nb, k, params, nullptr, nullptr, b.data(), db.data());
        all = all && std::memcmp(a.data(), b.data(), a.size() * 8) == 0 && std::memcmp(da.data(), db.data(), da.size() * 4) == 0;
    }
    std::printf("index==part %d\n", all ? 1 : 0);

    // wrong FixedString length: LOGICAL_ERROR
    const bool dimerr = throws(DB::ErrorCodes::LOGICAL_ERROR, [&] {
        index.search(q.data(), nq, nb - 1, k, "", nullptr, nullptr, b.data(), db.data());
    });
    std::printf("dimension %d\n", dimerr ? 1 : 0);

    // device failure: the caller's fallback serves the call; without one the
    // status is rethrown
    index.search(q.data(), nq, nb, k, "nprobe=12", nullptr, nullptr, a.data(), da.data());
    int served = 0;
    MI::BinaryGpuIndex::SearchFallback fb = [&](const uint8_t *, int32_t, int32_t, const std::string &, const uint8_t *,
                                               const uint8_t *, int64_t *ids, float *) {
        ++served;
        ids[0] = -42;
    };
    const uint64_t before = MI::fallbackCount().load();
    mqvs_inject_fault(MQVS_ERR_DEVICE, 1);
    index.search(q.data(), nq, nb, k, "nprobe=12", nullptr, nullptr, b.data(), db.data(), fb);
    bool fok = served == 1 && b[0] == -42 && MI::fallbackCount().load() == before + 1;
    mqvs_inject_fault(MQVS_ERR_MEMORY_LIMIT, 1);
    fok = fok && throws(DB::ErrorCodes::MEMORY_LIMIT_EXCEEDED, [&] {
              index.search(q.data(), nq, nb, k, "nprobe=12", nullptr, nullptr, b.data(), db.data());
          });
    mqvs_inject_fault(MQVS_ERR_DEVICE, 0);
    index.search(q.data(), nq, nb, k, "nprobe=12", nullptr, nullptr, b.data(), db.data());
    fok = fok && std::memcmp(a.data(), b.data(), a.size() * 8) == 0;
    std::printf("fallback %d\n", fok ? 1 : 0);

    // decoupled part: ids through the row_ids_map
    std::vector<uint64_t> map(n);
    for (int i = 0; i < n; ++i) map[i] = (uint64_t)((i * 7 + 3) % n);
    index.setRowIdsMap(map);
    index.search(q.data(), nq, nb, k, "nprobe=12", nullptr, nullptr, b.data(), db.data());
    bool mok = true;
    for (size_t i = 0; i < a.size(); ++i) mok = mok && b[i] == (a[i] >= 0 ? (int64_t)map[(size_t)a[i]] : -1) && db[i] == da[i];
    index.setRowIdsMap({});
    index.search(q.data(), nq, nb, k, "nprobe=12", nullptr, nullptr, b.data(), db.data());
    mok = mok && std::memcmp(a.data(), b.data(), a.size() * 8) == 0;
    std::printf("row_ids_map %d\n", mok ? 1 : 0);

    // a borrowed view searches the same index
    MI::BinaryGpuIndex view = MI::BinaryGpuIndex::borrow(MI::BinaryPartScan::borrow(part.handle()), index.handle());
    view.search(q.data(), nq, nb, k, "nprobe=12", nullptr, nullptr, b.data(), db.data());
    std::printf("borrow %d\n", std::memcmp(a.data(), b.data(), a.size() * 8) == 0 ? 1 : 0);
    return 0;
}

int main(int argc, char **argv) {
    try {
        if (argc >= 2 && std::string(argv[1]) == "errors") return errors();
        if (argc >= 2 && std::string(argv[1]) == "gpu") return gpu();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::fprintf(stderr, "usage: shim_binary_index errors | gpu\n");
    return 2;
}
