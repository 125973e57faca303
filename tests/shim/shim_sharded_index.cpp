// Compile-and-run check of the sharded-index part of include/mqvs_vector_index.hpp
// (GpuIndex::searchShard, ShardComm::searchIndex, ShardComm::loopback):
//   shim_sharded_index errors   no GPU needed: the argument checks' error mappings
//   shim_sharded_index gpu      a world-1 loopback communicator: searchIndex and
//                               searchShard (base -1) return GpuIndex::search's bits
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
    float q[4] = {0};
    int64_t ids[4];
    float dist[4];
    // (a null handle fails before any device work)
    bool ok = throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] {
        MI::check(mqvs_index_search_ex(nullptr, q, 1, 1, "", nullptr, nullptr, -1, ids, dist, 0, nullptr));
    });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] {
        MI::check(mqvs_index_search_ex(nullptr, q, 1, 1, "", nullptr, nullptr, (int64_t)1 << 31, ids, dist, 0, nullptr));
    });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] {
        MI::check(mqvs_sharded_index_search(nullptr, nullptr, q, 1, 1, "", nullptr, nullptr, ids, dist, 0, nullptr));
    });
    if (!ok) return 1;
    std::printf("errors ok\n");
    return 0;
}

static int gpu() {
    const int n = 4096, d = 48, nq = 6, k = 20;
    std::vector<float> rows((size_t)n * d), q((size_t)nq * d);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < d; ++j) rows[(size_t)i * d + j] = (float)((i * 37 + j * 11 + (i >> 4) * 5) % 97) / 16.0f - 3.0f;
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < d; ++j) q[(size_t)i * d + j] = rows[(size_t)(i * 600 + 3) * d + j] + (float)(j & 3) / 8.0f;
    MI::PartScan part(rows.data(), n, d, MQVS_METRIC_COSINE, 512, nullptr);
    MI::GpuIndex index(part, "MSTG", "nlist=10");
    const std::string params = "nprobe=3";
    std::vector<int64_t> a((size_t)nq * k), b((size_t)nq * k);
    std::vector<float> da((size_t)nq * k), db((size_t)nq * k);
    auto same = [&] {
        return std::memcmp(a.data(), b.data(), a.size() * 8) == 0 && std::memcmp(da.data(), db.data(), da.size() * 4) == 0;
    };
    index.search(q.data(), nq, d, k, params, nullptr, nullptr, false, a.data(), da.data());
    index.searchShard(q.data(), nq, d, k, params, nullptr, nullptr, -1, false, b.data(), db.data());
    std::printf("searchShard==search %d\n", same() ? 1 : 0);
    auto comms = MI::ShardComm::loopback(1, 0);
    bool all = true;
    for (int rep = 0; rep < 3; ++rep) {
        std::fill(b.begin(), b.end(), -7);
        comms[0]->searchIndex(index, q.data(), nq, k, params, nullptr, nullptr, false, b.data(), db.data());
        all = all && same();
    }
    std::printf("searchIndex==search %d\n", all ? 1 : 0);
    const auto st = comms[0]->stats();
    std::printf("fast %d\n", st.first == 2 && st.second == 0 ? 1 : 0);
    const bool bad = throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] {
        index.searchShard(q.data(), nq, d, k, params, nullptr, nullptr, (int64_t)1 << 31, false, b.data(), db.data());
    });
    std::printf("bad base %d\n", bad ? 1 : 0);
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
    std::fprintf(stderr, "usage: shim_sharded_index errors | gpu\n");
    return 2;
}
