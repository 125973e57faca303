// kernels_binary.hip -- brute-force scan of binary vectors (FixedString(N)
// columns): tryBruteForceSearch<BinaryVector> (BruteForceSearch.h:94-110),
// i.e. faiss::hammings_knn_mc (Hamming) and jaccard_knn (Jaccard) under
// vectorScanWithoutIndex<BinaryVector> (MergeTreeVSManager.cpp:1188-1273,
// 1395-1425).
//
// Popcount work is integer and HBM-bound (one 16-B code slice per lane per
// step, a handful of v_xor / v_bcnt per slice and query), so it stays on the
// VALU; no reshaping into MFMA.  A 256-thread workgroup owns a 256-row tile,
// one row per lane; code rows are 16-B aligned (stride code_words * 4 B, zero
// padded -- zero bytes add nothing to xor / and / or popcounts).  Queries are
// wave-uniform and come in through scalar loads, QC per pass; rows of up to
// 8 x 16 B (1024 bits) stay in registers across query passes, longer rows
// are re-read per pass (L1/L2 hits after the first).
//
// The value each row gets (the "raw" of the shared select pipeline):
//   Hamming  popcount(q ^ y) as a float; rows at distance == d bits are never
//            returned (hammings_knn_mc emits distances b < nBit only)
//   Jaccard  (den - num) / den in fp32, 1.0 when num == 0 (KAT 00038 pins the
//            division form)
// Both are ascending and finite, so probe / refine / final select run with
// the L2 ordering key (ord_asc) and the (key, row) tie rule of
// hammings_knn_mc's per-distance arrival order and searchWrapper's strict
// merge.  APPEND with tau_strict: after the probe (rows [0, P)) and every
// refine, the candidates hold every row scanned so far with key <= tau, and
// later segments only contain larger rows, so a row with key == tau can never
// beat the k-th candidate: strict `key < tau` keeps integer ties (Hamming)
// from flooding the candidate lists.
#include <cstdlib>

#include "flat_kernels.h"

namespace mqvs {

constexpr int kBinQC = 8;   // queries per pass (accumulators in registers)
constexpr int kBinRW = 8;   // 16-B slices kept in registers (REG: rows <= 1024 bits)

// ---------------------------------------------------------------------------
// A row's value has one definition: bin_popc and bin_probe_value are the
// expressions of every binary scan, the per-part kernels below and the grouped
// ones (k_scan_group_binary*).  The loop shells around them (bin_load_row,
// bin_row_pass, bin_co_popc) serve the grouped kernels only: they repeat the
// shells of k_scan_binary / k_scan_binary_co, which keep theirs in place --
// calling these from them changed their instruction streams (the REG form by
// some 280 instructions), calling the two value functions did not.

// one 16-B slice of a row against the same slice of a query
template <int METRIC>
__device__ __forceinline__ void bin_popc(const uint4 q, const uint4 y, uint32_t &a, uint32_t &b) {
    if (METRIC == MQVS_METRIC_HAMMING) {
        a += __builtin_popcount(q.x ^ y.x) + __builtin_popcount(q.y ^ y.y) +
             __builtin_popcount(q.z ^ y.z) + __builtin_popcount(q.w ^ y.w);
    } else {
        a += __builtin_popcount(q.x & y.x) + __builtin_popcount(q.y & y.y) +
             __builtin_popcount(q.z & y.z) + __builtin_popcount(q.w & y.w);
        b += __builtin_popcount(q.x | y.x) + __builtin_popcount(q.y | y.y) +
             __builtin_popcount(q.z | y.z) + __builtin_popcount(q.w | y.w);
    }
}

// (bin_probe_value, the dense PROBE value of a row: flat_kernels.h)

// row-per-lane form (k_scan_binary's load_row): the lane's row (position pos
// of a tile ending at r1) into registers, zeros past the tile
__device__ __forceinline__ void bin_load_row(const uint32_t *codes, int code_words, int W4, int64_t pos, int64_t r1,
                                             uint4 (&dst)[kBinRW]) {
    const uint4 *src = reinterpret_cast<const uint4 *>(codes + (pos < r1 ? pos : 0) * code_words);
#pragma unroll
    for (int u = 0; u < kBinRW; ++u) dst[u] = (u < W4 && pos < r1) ? src[u] : make_uint4(0u, 0u, 0u, 0u);
}

// row-per-lane form (k_scan_binary's query pass): the popcounts of kBinQC
// queries from j0 over the lane's row (REG: yc, else read from yr)
template <int METRIC, bool REG>
__device__ __forceinline__ void bin_row_pass(const ScanParams &p, int j0, int W4, const uint4 (&yc)[kBinRW],
                                             const uint4 *yr, bool inrange, uint32_t (&a)[kBinQC],
                                             uint32_t (&b)[kBinQC]) {
#pragma unroll
    for (int jj = 0; jj < kBinQC; ++jj) a[jj] = b[jj] = 0u;
    auto step = [&](const uint4 y, int u) {
#pragma unroll
        for (int jj = 0; jj < kBinQC; ++jj) {
            if (j0 + jj < p.nq) {  // wave-uniform
                const uint4 q = reinterpret_cast<const uint4 *>(p.qcodes + (int64_t)(j0 + jj) * p.code_words)[u];
                bin_popc<METRIC>(q, y, a[jj], b[jj]);
            }
        }
    };
    if (REG) {
#pragma unroll
        for (int u = 0; u < kBinRW; ++u)
            if (u < W4) step(yc[u], u);
    } else {
        for (int u = 0; u < W4; ++u) step(inrange ? yr[u] : make_uint4(0u, 0u, 0u, 0u), u);
    }
}

// coalesced form (k_scan_binary_co): slice yy of a row against query slice q,
// summed over the W4 lanes of the row
template <int METRIC, int W4>
__device__ __forceinline__ void bin_co_popc(const uint4 q, const uint4 yy, uint32_t &a, uint32_t &b) {
    a = b = 0u;
    bin_popc<METRIC>(q, yy, a, b);
#pragma unroll
    for (int o = 1; o < W4; o <<= 1) {
        a += __shfl_xor(a, o);
        if (METRIC == MQVS_METRIC_JACCARD) b += __shfl_xor(b, o);
    }
}

template <int METRIC, bool PROBE, bool REG>
__global__ __launch_bounds__(256) void k_scan_binary(ScanParams p) {
    constexpr int QC = 8;   // queries per pass (accumulators in registers)
    constexpr int RW = 8;   // 16-B slices kept in registers (REG: rows <= 1024 bits)
    const int t = threadIdx.x;
    const int W4 = p.code_words / 4;
    const int nbits = p.nbits;
    // REG: the next tile's row is loaded before this tile's popcounts, so two
    // rows per lane are in flight (HBM latency x bandwidth needs ~64 KB per CU)
    uint4 yn[RW];
    auto load_row = [&](int64_t ti, uint4 *dst) {
        int64_t r0, r1, chunk;
        tile_range(p, ti, r0, r1, chunk);
        const int64_t pos = r0 + t;
        const uint4 *src = reinterpret_cast<const uint4 *>(p.codes + (pos < r1 ? pos : 0) * p.code_words);
#pragma unroll
        for (int u = 0; u < RW; ++u) dst[u] = (u < W4 && pos < r1) ? src[u] : make_uint4(0u, 0u, 0u, 0u);
    };
    if (REG && blockIdx.x < p.tiles) load_row(blockIdx.x, yn);
    for (int64_t ti = blockIdx.x; ti < p.tiles; ti += gridDim.x) {
        int64_t r0, r1, chunk;
        tile_range(p, ti, r0, r1, chunk);
        const int64_t pos = r0 + t;
        const bool inrange = pos < r1;
        const int64_t row = pos;
        const bool valid_row = inrange && row_valid(p, row);
        const uint4 *yr = reinterpret_cast<const uint4 *>(p.codes + (inrange ? row : 0) * p.code_words);
        uint4 yc[RW];
        if (REG) {
#pragma unroll
            for (int u = 0; u < RW; ++u) yc[u] = yn[u];
            if (ti + gridDim.x < p.tiles) load_row(ti + gridDim.x, yn);
        }
        for (int j0 = 0; j0 < p.nq; j0 += QC) {
            uint32_t a[QC], b[QC];
#pragma unroll
            for (int jj = 0; jj < QC; ++jj) a[jj] = b[jj] = 0u;
            auto step = [&](const uint4 y, int u) {
#pragma unroll
                for (int jj = 0; jj < QC; ++jj) {
                    if (j0 + jj < p.nq) {  // wave-uniform
                        const uint4 q = reinterpret_cast<const uint4 *>(p.qcodes + (int64_t)(j0 + jj) * p.code_words)[u];
                        bin_popc<METRIC>(q, y, a[jj], b[jj]);
                    }
                }
            };
            if (REG) {
#pragma unroll
                for (int u = 0; u < RW; ++u)
                    if (u < W4) step(yc[u], u);
            } else {
                for (int u = 0; u < W4; ++u) step(inrange ? yr[u] : make_uint4(0u, 0u, 0u, 0u), u);
            }
#pragma unroll
            for (int jj = 0; jj < QC; ++jj) {
                const int j = j0 + jj;
                if (j >= p.nq) break;  // wave-uniform
                if (PROBE) {
                    const float v = bin_probe_value<METRIC>(a[jj], b[jj], valid_row, nbits);
                    if (inrange) p.probe[(int64_t)j * p.probe_ld + (pos - p.row_begin)] = v;
                    continue;
                }
                // APPEND: the threshold as a value (wave-uniform); keys of the
                // non-negative values are ord_asc = bits | 2^31, and a tau of
                // 0xFFFFFFFE / 0xFFFFFFFF (fewer than k rows so far) takes all
                const uint32_t tau = p.tau[j];
                const bool all = tau >= 0xFFFFFFFEu;
                const float tf = __builtin_bit_cast(float, tau & 0x7FFFFFFFu);
                bool take;
                float raw = 0.f;
                if (METRIC == MQVS_METRIC_HAMMING) {
                    // integer limit: h < ceil(tf) (strict) or h <= floor(tf)
                    int lim = nbits;
                    if (!all && tf < (float)nbits) lim = p.tau_strict ? (int)ceilf(tf) : (int)floorf(tf) + 1;
                    take = valid_row && (int)a[jj] < lim;
                    raw = (float)a[jj];
                } else {
                    // cheap superset test first, exact fp32 division for the few that pass
                    const float dn = (float)(b[jj] - a[jj]), dd = (float)b[jj];
                    take = valid_row && (all || a[jj] == 0u || dn <= tf * dd * 1.0000005f);
                    if (take) {
                        raw = a[jj] == 0u ? 1.0f : dn / dd;
                        const uint32_t key = ord_asc(raw);
                        take = p.tau_strict ? key < tau : key <= tau;
                    }
                }
                // (cand_append_wave, cand_list.h, kept open-coded: behind the
                // function this kernel compiles to another instruction stream)
                const unsigned long long m = __ballot(take);
                if (m == 0) continue;
                const int lane = t & 63;
                const int leader = __ffsll((long long)m) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&p.cand_count[j], __popcll(m));
                base = __shfl(base, leader);
                if (take) {
                    const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
                    cand_store(p.cand, p.cand_cap, j, slot, raw, (uint32_t)row);
                }
            }
        }
    }
}

// Small batches (nq <= 8) are HBM-bound: lanes read consecutive 16-B slices
// of the tile (fully coalesced) instead of one row each.  With W4 slices per
// row (W4 = 1, 2, 4, 8), lane t always holds slice u = t % W4 of rows
// (s * 256 + t) / W4, s = 0 .. W4-1; its query slices sit in registers for
// the whole launch, partial popcounts are summed over the W4 lanes of a row
// by xor-shuffles, and lane u == 0 emits the row.
template <int METRIC, bool PROBE, int W4>
__global__ __launch_bounds__(256) void k_scan_binary_co(ScanParams p) {
    constexpr int QC = 8;
    const int t = threadIdx.x;
    const int u = t & (W4 - 1);
    const int nbits = p.nq > 0 ? p.nbits : 0;
    uint4 qv[QC];
#pragma unroll
    for (int jj = 0; jj < QC; ++jj)
        qv[jj] = jj < p.nq ? reinterpret_cast<const uint4 *>(p.qcodes + (int64_t)jj * p.code_words)[u]
                           : make_uint4(0u, 0u, 0u, 0u);
    // per-query integer limits / value thresholds of APPEND (wave-uniform)
    int lim[QC];
    float tfv[QC];
    bool allv[QC];
#pragma unroll
    for (int jj = 0; jj < QC; ++jj) {
        lim[jj] = nbits;
        tfv[jj] = 0.f;
        allv[jj] = true;
        if (!PROBE && jj < p.nq) {
            const uint32_t tau = p.tau[jj];
            allv[jj] = tau >= 0xFFFFFFFEu;
            tfv[jj] = __builtin_bit_cast(float, tau & 0x7FFFFFFFu);
            if (!allv[jj] && tfv[jj] < (float)nbits)
                lim[jj] = p.tau_strict ? (int)ceilf(tfv[jj]) : (int)floorf(tfv[jj]) + 1;
        }
    }
    const uint4 *base = reinterpret_cast<const uint4 *>(p.codes);
    for (int64_t ti = blockIdx.x; ti < p.tiles; ti += gridDim.x) {
        int64_t r0, r1, chunk;
        tile_range(p, ti, r0, r1, chunk);
        uint4 y[W4];
#pragma unroll
        for (int sidx = 0; sidx < W4; ++sidx) {
            const int64_t row = r0 + (sidx * 256 + t) / W4;
            y[sidx] = row < r1 ? base[r0 * W4 + sidx * 256 + t] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int sidx = 0; sidx < W4; ++sidx) {
            const int64_t row = r0 + (sidx * 256 + t) / W4;
            const bool inrange = row < r1;
            const bool lead = u == 0;
            const bool valid_row = lead && inrange && row_valid(p, row);
#pragma unroll
            for (int jj = 0; jj < QC; ++jj) {
                if (jj >= p.nq) break;  // wave-uniform
                const uint4 q = qv[jj], yy = y[sidx];
                uint32_t a = 0u, b = 0u;
                bin_popc<METRIC>(q, yy, a, b);
#pragma unroll
                for (int o = 1; o < W4; o <<= 1) {
                    a += __shfl_xor(a, o);
                    if (METRIC == MQVS_METRIC_JACCARD) b += __shfl_xor(b, o);
                }
                if (PROBE) {
                    if (lead && inrange) {
                        p.probe[(int64_t)jj * p.probe_ld + (row - p.row_begin)] =
                            bin_probe_value<METRIC>(a, b, valid_row, nbits);
                    }
                    continue;
                }
                bool take;
                float raw = 0.f;
                if (METRIC == MQVS_METRIC_HAMMING) {
                    take = valid_row && (int)a < lim[jj];
                    raw = (float)a;
                } else {
                    const float dn = (float)(b - a), dd = (float)b;
                    take = valid_row && (allv[jj] || a == 0u || dn <= tfv[jj] * dd * 1.0000005f);
                    if (take) {
                        raw = a == 0u ? 1.0f : dn / dd;
                        const uint32_t key = ord_asc(raw);
                        const uint32_t tau = p.tau[jj];
                        take = p.tau_strict ? key < tau : key <= tau;
                    }
                }
                cand_append_wave(p.cand, p.cand_count, p.cand_cap, jj, take, raw, (uint32_t)row);
            }
        }
    }
}

static int64_t bin_grid_cap() {
    static const int64_t cap = [] {
        const char *e = tune_env("MQVS_BIN_GRID");  // tuning knob (tools/binary_sweep.py)
        return e ? std::max<int64_t>(64, std::atoll(e)) : (int64_t)4096;
    }();
    return cap;
}

// The form of a binary scan, per-part or grouped: launch(W4, REG) with W4 in
// {1, 2, 4, 8} for the coalesced kernel (small batches of those code widths),
// else W4 = 0 for the row-per-lane kernel, REG when its rows fit the registers.
template <class Launch>
static void bin_scan_form(const ScanParams &p, Launch &&launch) {
    const bool co = p.nq <= 8 && !tune_env("MQVS_BIN_NOCO");
    with_w4(co ? p.code_words : 0, [&](auto w4) {
        if (w4 > 0 || p.code_words <= 32)
            launch(w4, std::true_type{});
        else
            launch(w4, std::false_type{});
    });
}

template <int METRIC, bool PROBE>
static void scan_binary_t(const ScanParams &p, hipStream_t s) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(p.tiles, bin_grid_cap()));
    bin_scan_form(p, [&](auto w4, auto reg) {
        if constexpr (w4 > 0)
            hipLaunchKernelGGL((k_scan_binary_co<METRIC, PROBE, w4>), dim3(grid), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((k_scan_binary<METRIC, PROBE, reg>), dim3(grid), dim3(256), 0, s, p);
    });
}

void launch_scan_binary(const ScanParams &p, int metric, bool probe, hipStream_t s) {
    if (metric == MQVS_METRIC_HAMMING)
        probe ? scan_binary_t<MQVS_METRIC_HAMMING, true>(p, s) : scan_binary_t<MQVS_METRIC_HAMMING, false>(p, s);
    else
        probe ? scan_binary_t<MQVS_METRIC_JACCARD, true>(p, s) : scan_binary_t<MQVS_METRIC_JACCARD, false>(p, s);
}

// ---------------------------------------------------------------------------
// Part-group scan (part_group.hip, mqvs_part_group_search_binary): the PROBE
// form of the two scans above over many small parts in one launch, built as
// k_scan_group is from k_scan_small.  Tile ti of the launch belongs to the
// last slot with tile0 <= ti (slots[nslots] is the sentinel; slots without
// tiles are skipped); the workgroup takes that part's fields into its
// ScanParams and writes the part's dense values into columns [col0, col0 + n)
// of the launch's [nq][probe_ld] matrix.  The code width is the group's, so
// the form (coalesced / row per lane) holds across parts.  Binary parts need
// no chunk-aligned tiling (no per-chunk arithmetic): tiles of kSmallRows rows
// from row 0.
__device__ __forceinline__ const GroupSlot &bin_group_slot(const GroupSlot *slots, int nslots, int64_t ti) {
    int lo = 0, hi = nslots;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (slots[mid].tile0 <= ti) lo = mid;
        else hi = mid;
    }
    return slots[lo];
}

__device__ __forceinline__ void bin_group_take(ScanParams &p, const GroupSlot &g, float *matrix) {
    p.codes = g.codes;
    p.n = g.n;
    p.chunk_rows = g.granule;
    p.filter = g.filter;
    p.exists = g.exists;
    p.row_begin = 0;
    p.row_end = g.n;
    p.tiles_per_chunk = 0;
    p.tile_rows = kSmallRows;
    p.probe = matrix + g.col0;
}

template <int METRIC, bool REG>
__global__ __launch_bounds__(256) void k_scan_group_binary(ScanParams p, const GroupSlot *slots, int nslots,
                                                           int64_t tiles) {
    constexpr int QC = kBinQC, RW = kBinRW;
    const int t = threadIdx.x;
    const int W4 = p.code_words / 4;
    const int nbits = p.nbits;
    float *const matrix = p.probe;
    // REG: the next tile's row (of the next tile's part) is in flight during
    // this tile's popcounts, as in k_scan_binary
    uint4 yn[RW];
    auto load_row = [&](int64_t ti, uint4 (&dst)[RW]) {
        const GroupSlot &g = bin_group_slot(slots, nslots, ti);
        const int64_t r0 = (ti - g.tile0) * kSmallRows;
        const int64_t r1 = r0 + kSmallRows < g.n ? r0 + kSmallRows : g.n;
        bin_load_row(g.codes, p.code_words, W4, r0 + t, r1, dst);
    };
    if (REG && blockIdx.x < tiles) load_row(blockIdx.x, yn);
    for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        const GroupSlot &g = bin_group_slot(slots, nslots, ti);
        bin_group_take(p, g, matrix);
        int64_t r0, r1, chunk;
        tile_range(p, ti - g.tile0, r0, r1, chunk);
        const int64_t pos = r0 + t;
        const bool inrange = pos < r1;
        const bool valid_row = inrange && row_valid(p, pos);
        const uint4 *yr = reinterpret_cast<const uint4 *>(p.codes + (inrange ? pos : 0) * p.code_words);
        uint4 yc[RW];
        if (REG) {
#pragma unroll
            for (int u = 0; u < RW; ++u) yc[u] = yn[u];
            if (ti + gridDim.x < tiles) load_row(ti + gridDim.x, yn);
        }
        for (int j0 = 0; j0 < p.nq; j0 += QC) {
            uint32_t a[QC], b[QC];
            bin_row_pass<METRIC, REG>(p, j0, W4, yc, yr, inrange, a, b);
#pragma unroll
            for (int jj = 0; jj < QC; ++jj) {
                const int j = j0 + jj;
                if (j >= p.nq) break;  // wave-uniform
                if (inrange)
                    p.probe[(int64_t)j * p.probe_ld + pos] = bin_probe_value<METRIC>(a[jj], b[jj], valid_row, nbits);
            }
        }
    }
}

template <int METRIC, int W4>
__global__ __launch_bounds__(256) void k_scan_group_binary_co(ScanParams p, const GroupSlot *slots, int nslots,
                                                              int64_t tiles) {
    constexpr int QC = kBinQC;
    const int t = threadIdx.x;
    const int u = t & (W4 - 1);
    const int nbits = p.nq > 0 ? p.nbits : 0;
    float *const matrix = p.probe;
    uint4 qv[QC];
#pragma unroll
    for (int jj = 0; jj < QC; ++jj)
        qv[jj] = jj < p.nq ? reinterpret_cast<const uint4 *>(p.qcodes + (int64_t)jj * p.code_words)[u]
                           : make_uint4(0u, 0u, 0u, 0u);
    for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        const GroupSlot &g = bin_group_slot(slots, nslots, ti);
        bin_group_take(p, g, matrix);
        const uint4 *base = reinterpret_cast<const uint4 *>(p.codes);
        int64_t r0, r1, chunk;
        tile_range(p, ti - g.tile0, r0, r1, chunk);
        uint4 y[W4];
#pragma unroll
        for (int sidx = 0; sidx < W4; ++sidx) {
            const int64_t row = r0 + (sidx * 256 + t) / W4;
            y[sidx] = row < r1 ? base[r0 * W4 + sidx * 256 + t] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int sidx = 0; sidx < W4; ++sidx) {
            const int64_t row = r0 + (sidx * 256 + t) / W4;
            const bool inrange = row < r1;
            const bool lead = u == 0;
            const bool valid_row = lead && inrange && row_valid(p, row);
#pragma unroll
            for (int jj = 0; jj < QC; ++jj) {
                if (jj >= p.nq) break;  // wave-uniform
                uint32_t a, b;
                bin_co_popc<METRIC, W4>(qv[jj], y[sidx], a, b);
                if (lead && inrange)
                    p.probe[(int64_t)jj * p.probe_ld + row] = bin_probe_value<METRIC>(a, b, valid_row, nbits);
            }
        }
    }
}

template <int METRIC>
static void scan_group_binary_t(const ScanParams &p, const GroupSlot *slots, int nslots, int64_t tiles,
                                hipStream_t s) {
    const int64_t grid = tiles < 4096 ? tiles : 4096;
    if (grid < 1) return;
    bin_scan_form(p, [&](auto w4, auto reg) {
        if constexpr (w4 > 0)
            hipLaunchKernelGGL((k_scan_group_binary_co<METRIC, w4>), dim3((unsigned)grid), dim3(256), 0, s, p, slots,
                               nslots, tiles);
        else
            hipLaunchKernelGGL((k_scan_group_binary<METRIC, reg>), dim3((unsigned)grid), dim3(256), 0, s, p, slots,
                               nslots, tiles);
    });
}

void launch_scan_group_binary(const ScanParams &base, const GroupSlot *slots, int nslots, int64_t tiles, int metric,
                              hipStream_t s) {
    if (metric == MQVS_METRIC_HAMMING)
        scan_group_binary_t<MQVS_METRIC_HAMMING>(base, slots, nslots, tiles, s);
    else
        scan_group_binary_t<MQVS_METRIC_JACCARD>(base, slots, nslots, tiles, s);
}

// Hamming results of the faiss contract (mqvs_knn_binary_raw): float counts
// -> int32 in place (the reference's reinterpret_cast<int32_t*>(distance)),
// padding INT32_MAX.
__global__ void k_hamming_to_int(const int64_t *ids, float *dist, int64_t m) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        const int32_t v = ids[i] >= 0 ? (int32_t)dist[i] : 2147483647;
        reinterpret_cast<int32_t *>(dist)[i] = v;
    }
}

void launch_hamming_to_int(const int64_t *ids, float *dist, int64_t m, hipStream_t s) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, 1024));
    hipLaunchKernelGGL(k_hamming_to_int, dim3(grid), dim3(256), 0, s, ids, dist, m);
}

}  // namespace mqvs
