// Compile-and-run check of the persistence part of include/mqvs_vector_index.hpp
// (GpuIndex / BinaryGpuIndex serialize + load):
//   shim_index_persist errors   no GPU needed: mqvs_index_blob_info and the
//                               argument checks' error mappings
//   shim_index_persist gpu      serialize a GpuIndex, load it, compare one
//                               search; the same for a BinaryGpuIndex; a blob of
//                               another part is LOGICAL_ERROR
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
    uint8_t blob[128] = {0};
    size_t bytes = 0;
    mqvs_index_t h = nullptr;
    mqvs_index_blob_info_t info;
    bool ok = throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_index_save_size(nullptr, &bytes)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_index_save(nullptr, blob, 128, &bytes)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_index_load(nullptr, blob, 128, &h)); });
    // a stored first block of 64 zero bytes: no magic
    blob[16] = 0x02;
    blob[17] = 64 + 9;
    blob[21] = 64;
    ok = ok && throws(DB::ErrorCodes::ILLEGAL_COLUMN, [&] { MI::check(mqvs_index_blob_info(blob, 89, &info)); });
    ok = ok && throws(DB::ErrorCodes::ILLEGAL_COLUMN, [&] { MI::check(mqvs_index_blob_info(blob, 40, &info)); });
    blob[16] = 0x82;
    ok = ok && throws(DB::ErrorCodes::NOT_IMPLEMENTED, [&] { MI::check(mqvs_index_blob_info(blob, 89, &info)); });
    if (!ok) return 1;
    std::printf("errors ok\n");
    return 0;
}

static int gpu() {
    const int n = 4000, d = 48, nq = 6, k = 20;
    std::vector<float> rows((size_t)n * d), q((size_t)nq * d);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < d; ++j) rows[(size_t)i * d + j] = (float)((i * 37 + j * 11 + (i >> 4) * 5) % 97) / 16.0f - 3.0f;
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < d; ++j) q[(size_t)i * d + j] = rows[(size_t)(i * 600 + 3) * d + j] + (float)(j & 3) / 8.0f;
    MI::PartScan part(rows.data(), n, d, MQVS_METRIC_L2, 512, nullptr);
    std::vector<int64_t> a((size_t)nq * k), b((size_t)nq * k);
    std::vector<float> da((size_t)nq * k), db((size_t)nq * k);
    std::vector<uint8_t> blob;
    {
        MI::GpuIndex index(part, "MSTG", "nlist=10");
        index.search(q.data(), nq, d, k, "", nullptr, nullptr, false, a.data(), da.data());
        blob = index.serialize();
    }  // the built index is gone
    mqvs_index_blob_info_t info;
    MI::check(mqvs_index_blob_info(blob.data(), blob.size(), &info));
    std::printf("blob_info %d\n", info.n == n && info.dim == d && info.nlist == 10 && info.kind == MQVS_INDEX_KIND_FLOAT_IVF ? 1 : 0);
    MI::GpuIndex loaded = MI::GpuIndex::load(part, blob.data(), blob.size());
    loaded.search(q.data(), nq, d, k, "", nullptr, nullptr, false, b.data(), db.data());
    std::printf("float load==build %d\n",
                std::memcmp(a.data(), b.data(), a.size() * 8) == 0 && std::memcmp(da.data(), db.data(), da.size() * 4) == 0 ? 1 : 0);
    std::printf("reserialize %d\n", loaded.serialize() == blob ? 1 : 0);

    // a blob of another part: LOGICAL_ERROR (other rows: the fingerprint)
    rows[7] += 1.0f;
    MI::PartScan other(rows.data(), n, d, MQVS_METRIC_L2, 512, nullptr);
    const bool refused = throws(DB::ErrorCodes::LOGICAL_ERROR, [&] { MI::GpuIndex::load(other, blob.data(), blob.size()); });
    std::printf("other part %d\n", refused ? 1 : 0);

    const int bn = 3000, nb = 16;
    std::vector<uint8_t> codes((size_t)bn * nb), bq((size_t)nq * nb);
    for (int i = 0; i < bn; ++i)
        for (int j = 0; j < nb; ++j) codes[(size_t)i * nb + j] = (uint8_t)((i * 131 + j * 29 + (i >> 3) * 7) % 251);
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < nb; ++j) bq[(size_t)i * nb + j] = (uint8_t)(codes[(size_t)(i * 400 + 5) * nb + j] ^ (1u << (j & 7)));
    MI::BinaryPartScan bpart(codes.data(), bn, nb, MQVS_METRIC_HAMMING, 512);
    std::vector<uint8_t> bblob;
    {
        MI::BinaryGpuIndex index(bpart, "BINARYMSTG", "nlist=12");
        index.search(bq.data(), nq, nb, k, "", nullptr, nullptr, a.data(), da.data());
        bblob = index.serialize();
    }
    MI::BinaryGpuIndex bloaded = MI::BinaryGpuIndex::load(bpart, bblob.data(), bblob.size());
    bloaded.search(bq.data(), nq, nb, k, "", nullptr, nullptr, b.data(), db.data());
    std::printf("binary load==build %d\n",
                std::memcmp(a.data(), b.data(), a.size() * 8) == 0 && std::memcmp(da.data(), db.data(), da.size() * 4) == 0 ? 1 : 0);
    const bool kind = throws(DB::ErrorCodes::LOGICAL_ERROR, [&] { MI::GpuIndex::load(part, bblob.data(), bblob.size()); });
    std::printf("kind %d\n", kind ? 1 : 0);
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
    std::fprintf(stderr, "usage: shim_index_persist errors | gpu\n");
    return 2;
}
