// Compile-and-run check of the part-group part of include/mqvs_vector_index.hpp
// (PartGroup over PartScans):
//   shim_part_group errors   no GPU needed: the argument checks' error mappings
//   shim_part_group gpu      PartGroup::search over three parts == the per-part
//                            PartScan::search calls + mergePartResults, with the
//                            part labels of the winning rows
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
    int32_t part[4];
    int64_t ids[4];
    float dist[4];
    mqvs_part_group_t g = nullptr;
    mqvs_segment_t none[2] = {nullptr, nullptr};
    // (every one of these fails before any device work)
    bool ok = throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_part_group_create(none, 0, &g)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_part_group_create(none, 2, &g)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::check(mqvs_part_group_create(none, 2, nullptr)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] {
        MI::check(mqvs_part_group_search(nullptr, q, 1, 1, MQVS_METRIC_L2, nullptr, nullptr, part, ids, dist, 0, nullptr));
    });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS,
                      [&] { MI::check(mqvs_part_group_info(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS, [&] { MI::PartGroup empty(std::vector<const MI::PartScan *>{}); });
    ok = ok && throws(DB::ErrorCodes::BAD_ARGUMENTS,
                      [&] { MI::PartGroup null_part(std::vector<const MI::PartScan *>{nullptr}); });
    if (!ok) return 1;
    std::printf("errors ok\n");
    return 0;
}

static int gpu() {
    const int d = 24, nq = 3, k = 30, np = 3;
    const int n[np] = {700, 257, 2000};
    std::vector<std::vector<float>> rows(np);
    std::vector<MI::PartScan> parts;
    for (int p = 0; p < np; ++p) {
        rows[p].resize((size_t)n[p] * d);
        // small integers (equal scores within and across parts), scrambled so
        // that the best rows come from more than one part
        for (int i = 0; i < n[p]; ++i)
            for (int j = 0; j < d; ++j) {
                const uint32_t h = ((uint32_t)i * 2654435761u + (uint32_t)j * 40503u + (uint32_t)p * 977u) * 2246822519u;
                rows[p][(size_t)i * d + j] = (float)((h >> 13) % 9u) - 4.0f;
            }
        parts.emplace_back(rows[p].data(), n[p], d, MQVS_METRIC_IP, 256, nullptr);
    }
    std::vector<float> q((size_t)nq * d);
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < d; ++j) q[(size_t)i * d + j] = (float)((i + j) % 3) - 1.0f;
    // part 1 carries a lightweight-delete mask with every third row deleted
    std::vector<uint8_t> ex((n[1] + 7) / 8, 0);
    for (int i = 0; i < n[1]; ++i)
        if (i % 3) ex[i >> 3] |= (uint8_t)(1u << (i & 7));
    const uint8_t *exists[np] = {nullptr, ex.data(), nullptr};

    std::vector<int64_t> li((size_t)np * nq * k), mi((size_t)nq * k), gi((size_t)nq * k);
    std::vector<float> ld(li.size()), md(mi.size()), gd(mi.size());
    std::vector<int32_t> gp(mi.size());
    for (int p = 0; p < np; ++p)
        parts[p].search(q.data(), nq, k, nullptr, exists[p], li.data() + (size_t)p * nq * k, ld.data() + (size_t)p * nq * k);
    MI::mergePartResults(np, nq, k, MQVS_METRIC_IP, li.data(), ld.data(), mi.data(), md.data());

    MI::PartGroup group({&parts[0], &parts[1], &parts[2]});
    group.search(q.data(), nq, k, nullptr, exists, gp.data(), gi.data(), gd.data());
    const bool same = std::memcmp(mi.data(), gi.data(), mi.size() * 8) == 0 &&
                      std::memcmp(md.data(), gd.data(), md.size() * 4) == 0;
    std::printf("group==loop %d\n", same ? 1 : 0);
    // a label is right when the part's own list holds (id, distance bits) for the query
    bool labels = true;
    int seen[np] = {0, 0, 0};
    for (int qi = 0; qi < nq; ++qi)
        for (int i = 0; i < k; ++i) {
            const size_t o = (size_t)qi * k + i;
            if (gi[o] < 0) {
                labels = labels && gp[o] == -1;
                continue;
            }
            const int p = gp[o];
            bool found = false;
            if (p >= 0 && p < np)
                for (int j = 0; j < k && !found; ++j) {
                    const size_t lo = ((size_t)p * nq + qi) * k + j;
                    found = li[lo] == gi[o] && std::memcmp(&ld[lo], &gd[o], 4) == 0;
                }
            if (!found && labels)
                std::printf("query %d slot %d: part %d does not list id %lld\n", qi, i, p, (long long)gi[o]);
            labels = labels && found;
            if (found) seen[p] = 1;
        }
    std::printf("labels %d\n", labels && seen[0] + seen[1] + seen[2] >= 2 ? 1 : 0);
    const mqvs_part_group_stats st = MI::PartGroup::lastStats();
    std::printf("fused %d\n", st.parts == 3 && st.fused_parts == 3 && st.looped_parts == 0 ? 1 : 0);
    const MI::PartRows pr = group.search(q.data(), nq, d, k, nullptr, exists);
    // (the labelled rows are the raw result with its padding slots dropped)
    size_t valid = 0;
    for (int64_t id : gi) valid += id >= 0;
    bool rows_ok = valid > 0 && pr.part.size() == valid && pr.label.size() == valid && pr.distance.size() == valid &&
                   pr.vector_id.size() == valid;
    for (size_t i = 0, j = 0; rows_ok && i < gi.size(); ++i) {
        if (gi[i] < 0) continue;
        rows_ok = pr.part[j] == (uint32_t)gp[i] && pr.label[j] == (uint32_t)gi[i] && pr.vector_id[j] == i / k &&
                  std::memcmp(&pr.distance[j], &gd[i], 4) == 0;
        ++j;
    }
    std::printf("rows %d\n", rows_ok ? 1 : 0);
    const bool dim = throws(DB::ErrorCodes::LOGICAL_ERROR, [&] { (void)group.search(q.data(), nq, d + 1, k); });
    std::printf("bad dim %d\n", dim ? 1 : 0);
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
    std::fprintf(stderr, "usage: shim_part_group errors | gpu\n");
    return 2;
}
