// kernels_bivf.hip -- the binary vector index (BINARYMSTG seam): an inverted
// file over k-majority (Hamming k-means) lists of FixedString codes.
//
// Everything here is integer arithmetic (popcounts; for Jaccard one fp32
// division of two integers, the expression of kernels_binary.hip), so the
// list scan computes the final distance: no approximate stage and no re-rank.
//
// Build     k_bivf_assign    nearest centroid by Hamming distance, ties to the
//                            lowest list id (rows of the sample, then all rows);
//                            assign=mfma: k_bivf_assign_mfma, which shares its
//                            tile body with the batch scan and lives beside
//                            it in kernels_binary_mfma.hip
//           k_bivf_count     per (list, bit) member counts (integer atomics:
//                            order-independent, so the build is deterministic)
//           k_bivf_majority  centroid bit = 2 ones > members; empty lists keep
//           k_bivf_gather    rows by an index list (sample, initial centroids,
//                            the list-ordered copy of the codes)
// Search    k_bivf_cdist     Hamming distance of every (query, centroid)
//           k_bivf_pick      the nprobe nearest lists by (distance, list id):
//                            two radix selects (k-th distance, then the list id
//                            bound inside the tie group)
//           k_bivf_scan      (query, probed list, 256-position slice) work
//                            items; every kept position appends one 8-B record
//                            (value, part row) to its query's region, which
//                            launch_final_select -- the brute-force path's
//                            final select -- orders by (distance, row)
//
// Code rows are [code_words] 32-bit words, 16-B aligned and zero padded, in
// the segment and in the list-ordered copy alike.
#include <cstdlib>

#include "index_kernels.h"
#include "select_common.h"

namespace mqvs {

typedef uint32_t bivf_u32x4 __attribute__((ext_vector_type(4)));

__device__ inline uint32_t pop_xor(const bivf_u32x4 q, const bivf_u32x4 y) {
    return __builtin_popcount(q[0] ^ y[0]) + __builtin_popcount(q[1] ^ y[1]) + __builtin_popcount(q[2] ^ y[2]) +
           __builtin_popcount(q[3] ^ y[3]);
}
__device__ inline uint32_t pop_and(const bivf_u32x4 q, const bivf_u32x4 y) {
    return __builtin_popcount(q[0] & y[0]) + __builtin_popcount(q[1] & y[1]) + __builtin_popcount(q[2] & y[2]) +
           __builtin_popcount(q[3] & y[3]);
}
__device__ inline uint32_t pop_or(const bivf_u32x4 q, const bivf_u32x4 y) {
    return __builtin_popcount(q[0] | y[0]) + __builtin_popcount(q[1] | y[1]) + __builtin_popcount(q[2] | y[2]) +
           __builtin_popcount(q[3] | y[3]);
}

// ---- build ------------------------------------------------------------------

// assign[r] = the centroid at the smallest Hamming distance of row r, the
// lowest list id among equals (a centroid at distance == nbits is a
// legitimate nearest list).  One row per lane; the centroid words are
// wave-uniform.  REG: rows of up to 8 x 16 B stay in registers.
template <bool REG>
__global__ __launch_bounds__(256) void k_bivf_assign(const uint32_t *codes, int64_t n, int code_words,
                                                     const uint32_t *cent, int nlist, int32_t *assign) {
    constexpr int RW = 8;
    const int W4 = code_words / 4;
    for (int64_t r = blockIdx.x * 256ll + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const bivf_u32x4 *y = reinterpret_cast<const bivf_u32x4 *>(codes + r * code_words);
        bivf_u32x4 yc[RW];
        if (REG) {
#pragma unroll
            for (int u = 0; u < RW; ++u) yc[u] = u < W4 ? y[u] : bivf_u32x4{0u, 0u, 0u, 0u};
        }
        uint32_t best = 0xFFFFFFFFu;
        int32_t arg = 0;
        for (int c = 0; c < nlist; ++c) {
            const bivf_u32x4 *cc = reinterpret_cast<const bivf_u32x4 *>(cent + (int64_t)c * code_words);
            uint32_t a = 0;
            if (REG) {
#pragma unroll
                for (int u = 0; u < RW; ++u)
                    if (u < W4) a += pop_xor(cc[u], yc[u]);
            } else {
                for (int u = 0; u < W4; ++u) a += pop_xor(cc[u], y[u]);
            }
            if (a < best) {
                best = a;
                arg = c;
            }
        }
        assign[r] = arg;
    }
}

void launch_bivf_assign(const uint32_t *codes, int64_t n, int code_words, const uint32_t *cent, int nlist,
                        int32_t *assign, hipStream_t s) {
    if (n <= 0) return;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 1 << 20);
    if (code_words <= 32)
        hipLaunchKernelGGL(k_bivf_assign<true>, dim3(grid), dim3(256), 0, s, codes, n, code_words, cent, nlist, assign);
    else
        hipLaunchKernelGGL(k_bivf_assign<false>, dim3(grid), dim3(256), 0, s, codes, n, code_words, cent, nlist,
                           assign);
}

// counts[(list * code_words + w) * 32 + b] += 1 for every set bit b of word w
// of a member row; members[list] += 1 per row
__global__ __launch_bounds__(256) void k_bivf_count(const uint32_t *codes, int64_t m, int code_words,
                                                    const int32_t *assign, int nlist, uint32_t *counts,
                                                    uint32_t *members) {
    const int64_t total = m * code_words;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / code_words;
        const int w = (int)(i % code_words);
        const int32_t a = assign[r];
        if (a < 0 || a >= nlist) continue;
        if (w == 0) atomicAdd(&members[a], 1u);
        uint32_t word = codes[i];
        uint32_t *dst = counts + ((int64_t)a * code_words + w) * 32;
        while (word) {
            const int b = __ffs((int)word) - 1;
            atomicAdd(&dst[b], 1u);
            word &= word - 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_bivf_majority(const uint32_t *counts, const uint32_t *members, int nlist,
                                                       int code_words, uint32_t *cent) {
    const int64_t total = (int64_t)nlist * code_words;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const uint32_t mem = members[i / code_words];
        if (mem == 0) continue;  // a list with no members keeps its centroid
        uint32_t word = 0;
        for (int b = 0; b < 32; ++b) word |= (2u * counts[i * 32 + b] > mem ? 1u : 0u) << b;
        cent[i] = word;
    }
}

void launch_bivf_majority(const uint32_t *codes, int64_t m, int code_words, const int32_t *assign, int nlist,
                          uint32_t *counts, uint32_t *members, uint32_t *cent, hipStream_t s) {
    const int64_t total = m * code_words;
    if (total > 0) {
        const int grid = (int)std::min<int64_t>((total + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(k_bivf_count, dim3(grid), dim3(256), 0, s, codes, m, code_words, assign, nlist, counts,
                           members);
    }
    const int64_t cw = (int64_t)nlist * code_words;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((cw + 255) / 256, 1 << 20));
    hipLaunchKernelGGL(k_bivf_majority, dim3(grid), dim3(256), 0, s, counts, members, nlist, code_words, cent);
}

// dst[pos] = src[idx[pos]] (16-B slices; idx < 0: zeros)
__global__ __launch_bounds__(256) void k_bivf_gather(const uint32_t *src, int code_words, const int32_t *idx,
                                                     int64_t m, uint32_t *dst) {
    const int W4 = code_words / 4;
    const int64_t total = m * W4;
    const bivf_u32x4 *s4 = reinterpret_cast<const bivf_u32x4 *>(src);
    bivf_u32x4 *d4 = reinterpret_cast<bivf_u32x4 *>(dst);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t pos = i / W4;
        const int u = (int)(i % W4);
        const int32_t r = idx[pos];
        d4[i] = r >= 0 ? s4[(int64_t)r * W4 + u] : bivf_u32x4{0u, 0u, 0u, 0u};
    }
}

void launch_bivf_gather(const uint32_t *src, int code_words, const int32_t *idx, int64_t m, uint32_t *dst,
                        hipStream_t s) {
    const int64_t total = m * (code_words / 4);
    if (total <= 0) return;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(k_bivf_gather, dim3(grid), dim3(256), 0, s, src, code_words, idx, m, dst);
}

// ---- coarse -----------------------------------------------------------------

// the Hamming distance of query row qq and centroid row cc ([W4] 16-B slices)
__device__ __forceinline__ uint32_t bivf_cdist_one(const uint32_t *qq, const uint32_t *cc, int W4) {
    const bivf_u32x4 *c4 = reinterpret_cast<const bivf_u32x4 *>(cc);
    const bivf_u32x4 *q4 = reinterpret_cast<const bivf_u32x4 *>(qq);
    uint32_t a = 0;
    for (int u = 0; u < W4; ++u) a += pop_xor(q4[u], c4[u]);
    return a;
}

__global__ __launch_bounds__(256) void k_bivf_cdist(const uint32_t *cent, int nlist, int code_words,
                                                    const uint32_t *qcodes, int nq, uint32_t *out) {
    const int W4 = code_words / 4;
    const int64_t tpq = (nlist + 255) / 256;
    const int64_t tiles = tpq * nq;
    for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        const int q = (int)(ti / tpq);
        const int c = (int)(ti % tpq) * 256 + threadIdx.x;
        if (c >= nlist) continue;
        out[(int64_t)q * nlist + c] =
            bivf_cdist_one(qcodes + (int64_t)q * code_words, cent + (int64_t)c * code_words, W4);
    }
}

// out[0, nprobe) = the nprobe lists of smallest (distance, list id) among
// d[0, nlist), in no particular order; nprobe < nlist.  The whole workgroup
// calls it (k_bivf_pick and the grouped pick: the rule is stated once).
// hist[256], sh[4], s_cnt_p: LDS words.
__device__ __forceinline__ void bivf_pick_body(const uint32_t *d, int nlist, int nprobe, int64_t *out, uint32_t *hist,
                                               uint32_t *sh, int *s_cnt_p) {
    int &s_cnt = *s_cnt_p;
    const uint32_t th = block_radix_select_mlp([&](int64_t i) { return d[i]; }, nlist, nprobe, hist, sh);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int below = 0;
    for (int i = threadIdx.x; i < nlist; i += SEL_THREADS) below += d[i] < th;
    atomicAdd(&s_cnt, below);
    __syncthreads();
    const int nbelow = s_cnt;
    __syncthreads();
    const uint32_t lth = block_radix_select_mlp([&](int64_t i) { return d[i] == th ? (uint32_t)i : 0xFFFFFFFFu; },
                                                nlist, nprobe - nbelow, hist, sh);
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < nlist; i += SEL_THREADS) {
        const uint32_t v = d[i];
        if (v < th || (v == th && (uint32_t)i <= lth)) {
            const int slot = atomicAdd(&s_cnt, 1);
            if (slot < nprobe) out[slot] = i;
        }
    }
}

// probes[q][0, nprobe) = the nprobe lists of smallest (distance, list id), in
// no particular order; nprobe < nlist
__global__ __launch_bounds__(SEL_THREADS) void k_bivf_pick(const uint32_t *cdist, int nlist, int nprobe,
                                                           int64_t *probes) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[4];
    __shared__ int s_cnt;
    const int q = blockIdx.x;
    bivf_pick_body(cdist + (int64_t)q * nlist, nlist, nprobe, probes + (int64_t)q * nprobe, hist, sh, &s_cnt);
}

void launch_bivf_coarse(const uint32_t *cent, int nlist, int code_words, const uint32_t *qcodes, int nq, int nprobe,
                        uint32_t *cdist, int64_t *probes, hipStream_t s) {
    if (nq <= 0) return;
    const int64_t tiles = (int64_t)((nlist + 255) / 256) * nq;
    hipLaunchKernelGGL(k_bivf_cdist, dim3((unsigned)std::min<int64_t>(tiles, 1 << 20)), dim3(256), 0, s, cent, nlist,
                       code_words, qcodes, nq, cdist);
    hipLaunchKernelGGL(k_bivf_pick, dim3(nq), dim3(SEL_THREADS), 0, s, cdist, nlist, nprobe, probes);
}

// ---- list scan --------------------------------------------------------------

// The record of a kept position: the final distance and the part row (the
// final select's tie order is the row, so it is read through perm here).
template <int METRIC>
__device__ inline void bivf_emit(const BivfParams &p, int q, bool lead, int64_t pos, uint32_t a, uint32_t b) {
    bool take = false;
    float raw = 0.f;
    uint32_t row = 0;
    if (lead) {
        const int32_t r = p.perm[pos];
        take = r >= 0;
        if (take && p.filter && !bit_test(p.filter, r)) take = false;
        if (take && p.exists && !bit_test(p.exists, r)) take = false;
        row = (uint32_t)r;
        if (METRIC == MQVS_METRIC_HAMMING) {
            raw = (float)a;
            take = take && (int)a < p.nbits;  // hammings_knn_mc emits distances b < nBit only
        } else {
            raw = a == 0u ? 1.0f : (float)(b - a) / (float)b;
        }
    }
    // (cand_append_wave, cand_list.h, kept open-coded: behind the function the
    // W4 = 1 scans compile with other registers)
    const unsigned long long m = __ballot(take);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&p.cand_count[q], __popcll(m));
    base = __shfl(base, leader);
    if (take) cand_store(p.cand, p.cand_cap, q, base + __popcll(m & ((1ull << lane) - 1ull)), raw, row);
}

// W4 = 1, 2, 4, 8: lanes read consecutive 16-B slices of the list (fully
// coalesced, as k_scan_binary_co): lane t holds slice t % W4 of position
// (s * 256 + t) / W4, the query's slice stays in a register for the item, and
// partial popcounts are combined by xor-shuffles.  W4 = 0: a position per
// lane (rows of other widths), the query's slices wave-uniform.
template <int METRIC, int W4>
__device__ __forceinline__ void bivf_scan_item(const BivfParams &p, int q, int64_t list, int ch) {
    const int t = threadIdx.x;
    const bivf_u32x4 *plane = reinterpret_cast<const bivf_u32x4 *>(p.plane);
    if (list < 0 || list >= p.nlist) return;  // (block-uniform)
    const int64_t b0 = p.list_off[list] + (int64_t)ch * 256, le = p.list_off[list + 1];
    if (b0 >= le) return;
    const int64_t e0 = le < b0 + 256 ? le : b0 + 256;
    if (W4 > 0) {
        const int u = t & (W4 - 1);
        const bivf_u32x4 qv = reinterpret_cast<const bivf_u32x4 *>(p.qcodes + (int64_t)q * p.code_words)[u];
        bivf_u32x4 y[W4 > 0 ? W4 : 1];
#pragma unroll
        for (int sidx = 0; sidx < W4; ++sidx) {
            const int idx = sidx * 256 + t;
            const int64_t pos = b0 + idx / W4;
            y[sidx] = pos < e0 ? __builtin_nontemporal_load(plane + b0 * W4 + idx) : bivf_u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int sidx = 0; sidx < W4; ++sidx) {
            const int64_t pos = b0 + (sidx * 256 + t) / W4;
            uint32_t a, b = 0u;
            if (METRIC == MQVS_METRIC_HAMMING) {
                a = pop_xor(qv, y[sidx]);
            } else {
                a = pop_and(qv, y[sidx]);
                b = pop_or(qv, y[sidx]);
            }
#pragma unroll
            for (int o = 1; o < W4; o <<= 1) {
                a += __shfl_xor(a, o);
                if (METRIC == MQVS_METRIC_JACCARD) b += __shfl_xor(b, o);
            }
            bivf_emit<METRIC>(p, q, u == 0 && pos < e0, pos, a, b);
        }
    } else {
        const int W = p.code_words / 4;
        const int64_t pos = b0 + t;
        const bool in = pos < e0;
        const bivf_u32x4 *yr = plane + (in ? pos : b0) * W;
        const bivf_u32x4 *qr = reinterpret_cast<const bivf_u32x4 *>(p.qcodes + (int64_t)q * p.code_words);
        uint32_t a = 0u, b = 0u;
        for (int u = 0; u < W; ++u) {
            const bivf_u32x4 yy = __builtin_nontemporal_load(yr + u), qq = qr[u];
            if (METRIC == MQVS_METRIC_HAMMING) {
                a += pop_xor(qq, yy);
            } else {
                a += pop_and(qq, yy);
                b += pop_or(qq, yy);
            }
        }
        bivf_emit<METRIC>(p, q, in, pos, a, b);
    }
}

template <int METRIC, int W4>
__global__ __launch_bounds__(256) void k_bivf_scan(BivfParams p) {
    const int64_t items = (int64_t)p.nq * p.nprobe * p.nch;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int ch = (int)(it % p.nch);
        const int64_t pair = it / p.nch;
        bivf_scan_item<METRIC, W4>(p, (int)(pair / p.nprobe), p.probes[pair], ch);
    }
}

template <int METRIC>
static void bivf_scan_t(const BivfParams &p, int grid, hipStream_t s) {
    with_w4(p.code_words, [&](auto w4) {
        hipLaunchKernelGGL((k_bivf_scan<METRIC, w4>), dim3(grid), dim3(256), 0, s, p);
    });
}

// stats[0] records written, [1] non-empty work items, [2] list-plane bytes of
// the probed lists, [3] (query, list) pairs
__global__ __launch_bounds__(256) void k_bivf_stats(BivfParams p, int64_t *stats) {
    __shared__ unsigned long long acc[3];
    if (threadIdx.x < 3) acc[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long vals = 0, items = 0, pos = 0;
    for (int i = threadIdx.x; i < p.nq; i += 256) vals += (unsigned long long)p.cand_count[i];
    const int64_t E = (int64_t)p.nq * p.nprobe;
    for (int64_t e = threadIdx.x; e < E; e += 256) {
        const int64_t list = p.probes[e];
        if (list < 0 || list >= p.nlist) continue;
        const int64_t len = p.list_off[list + 1] - p.list_off[list];
        pos += (unsigned long long)len;
        items += (unsigned long long)((len + 255) / 256);
    }
    atomicAdd(&acc[0], vals);
    atomicAdd(&acc[1], items);
    atomicAdd(&acc[2], pos);
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[0] = (int64_t)acc[0];
        stats[1] = (int64_t)acc[1];
        stats[2] = (int64_t)acc[2] * p.code_words * 4;
        stats[3] = E;
    }
}

void launch_bivf_scan(const BivfParams &p, int metric, int64_t *stats, hipStream_t s) {
    const int64_t items = (int64_t)p.nq * p.nprobe * p.nch;
    if (items > 0) {
        const int grid = (int)std::min<int64_t>(items, 1 << 16);
        if (metric == MQVS_METRIC_HAMMING)
            bivf_scan_t<MQVS_METRIC_HAMMING>(p, grid, s);
        else
            bivf_scan_t<MQVS_METRIC_JACCARD>(p, grid, s);
    }
    if (stats) hipLaunchKernelGGL(k_bivf_stats, dim3(1), dim3(256), 0, s, p, stats);
}

// ---- index groups (index_group.hip) -------------------------------------------
// The search kernels above with a batch dimension over the indexed parts of a
// group: one slot per part (BivfGroupSlot, index_kernels.h).  A workgroup's
// work unit v belongs to the last slot whose prefix sum (ctile0 / item0) is
// <= v -- the table ends with a sentinel holding the totals, and slots without
// units are skipped -- which depends on blockIdx only, so it is wave-uniform.
__device__ __forceinline__ int bivf_group_slot(const BivfGroupSlot *slots, int nslots, int64_t v,
                                               int64_t BivfGroupSlot::*key) {
    int lo = 0, hi = nslots;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (slots[mid].*key <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// k_bivf_cdist over the 256-centroid tiles of every (ranked slot, query):
// cdist[q][cent0 + c] of the slice's [nq][ld] matrix
__global__ __launch_bounds__(256) void k_bivf_group_cdist(const BivfGroupSlot *slots, int nslots, int64_t tiles,
                                                          int code_words, const uint32_t *qcodes, uint32_t *cdist,
                                                          int64_t ld) {
    const int W4 = code_words / 4;
    for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        const BivfGroupSlot &g = slots[bivf_group_slot(slots, nslots, ti, &BivfGroupSlot::ctile0)];
        const int64_t local = ti - g.ctile0;
        const int64_t tpq = (g.nlist + 255) / 256;
        const int q = (int)(local / tpq);
        const int c = (int)(local % tpq) * 256 + threadIdx.x;
        if (c >= g.nlist) continue;
        cdist[(int64_t)q * ld + g.cent0 + c] =
            bivf_cdist_one(qcodes + (int64_t)q * code_words, g.bcent + (int64_t)c * code_words, W4);
    }
}

// workgroup (slot, query): the slot's probes of the query -- k_bivf_pick's
// rule over the slot's columns, or every list in order when the slot probes
// all of them -- and the (slot, query) record counter zeroed for the scan
__global__ __launch_bounds__(SEL_THREADS) void k_bivf_group_pick(const BivfGroupSlot *slots, int nq,
                                                                 const uint32_t *cdist, int64_t ld, int64_t *probes,
                                                                 int *count) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh[4];
    __shared__ int s_cnt;
    const int q = blockIdx.x % nq;
    const BivfGroupSlot &g = slots[blockIdx.x / nq];
    int64_t *out = probes + g.probe0 + (int64_t)q * g.nprobe;
    if (threadIdx.x == 0) count[g.count0 + q] = 0;
    if (g.nprobe < g.nlist) {  // (block-uniform)
        bivf_pick_body(cdist + (int64_t)q * ld + g.cent0, g.nlist, g.nprobe, out, hist, sh, &s_cnt);
    } else {
        for (int r = threadIdx.x; r < g.nprobe; r += SEL_THREADS) out[r] = r;
    }
}

// k_bivf_scan's work items of every slot: item it of the launch is (query,
// probe, 256-position slice) it - item0 of its slot; the records go to the
// (slot, query) region cand[cand0 + q cap ..) under count[count0 + q]
template <int METRIC, int W4>
__global__ __launch_bounds__(256) void k_bivf_group_scan(BivfParams base, const BivfGroupSlot *slots, int nslots,
                                                         int64_t items, int *count) {
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const BivfGroupSlot &g = slots[bivf_group_slot(slots, nslots, it, &BivfGroupSlot::item0)];
        const int64_t local = it - g.item0;
        const int ch = (int)(local % g.nch);
        const int64_t pair = local / g.nch;
        BivfParams p = base;
        p.plane = g.bplane;
        p.perm = g.perm;
        p.list_off = g.list_off;
        p.nlist = g.nlist;
        p.filter = g.filter;
        p.exists = g.exists;
        p.cand = base.cand + g.cand0;
        p.cand_count = count + g.count0;
        p.cand_cap = g.cap;
        bivf_scan_item<METRIC, W4>(p, (int)(pair / g.nprobe), base.probes[g.probe0 + pair], ch);
    }
}

template <int METRIC>
static void bivf_group_scan_t(const BivfParams &p, const BivfGroupSlot *slots, int nslots, int64_t items, int *count,
                              int grid, hipStream_t s) {
    with_w4(p.code_words, [&](auto w4) {
        hipLaunchKernelGGL((k_bivf_group_scan<METRIC, w4>), dim3(grid), dim3(256), 0, s, p, slots, nslots, items,
                           count);
    });
}

void launch_bivf_group_coarse(const BivfGroupSlot *slots, int nslots, int64_t ctiles, int code_words,
                              const uint32_t *qcodes, int nq, uint32_t *cdist, int64_t ld, int64_t *probes, int *count,
                              hipStream_t s) {
    if (nq <= 0 || nslots <= 0) return;
    if (ctiles > 0)
        hipLaunchKernelGGL(k_bivf_group_cdist, dim3((unsigned)std::min<int64_t>(ctiles, 1 << 20)), dim3(256), 0, s,
                           slots, nslots, ctiles, code_words, qcodes, cdist, ld);
    hipLaunchKernelGGL(k_bivf_group_pick, dim3((unsigned)nslots * nq), dim3(SEL_THREADS), 0, s, slots, nq, cdist, ld,
                       probes, count);
}

void launch_bivf_group_scan(const BivfParams &base, const BivfGroupSlot *slots, int nslots, int64_t items, int *count,
                            int metric, hipStream_t s) {
    if (items <= 0 || nslots <= 0) return;
    const int grid = (int)std::min<int64_t>(items, 1 << 16);
    if (metric == MQVS_METRIC_HAMMING)
        bivf_group_scan_t<MQVS_METRIC_HAMMING>(base, slots, nslots, items, count, grid, s);
    else
        bivf_group_scan_t<MQVS_METRIC_JACCARD>(base, slots, nslots, items, count, grid, s);
}

// workgroup (table entry, one of bx blocks over the entry's nq * k results):
// ids through the part's row-ids map, as k_map_ids; slots without a map (and
// sentinels) return
__global__ __launch_bounds__(256) void k_bivf_group_map(const BivfGroupSlot *slots, int bx, int64_t per_part,
                                                        int64_t *list_ids) {
    const BivfGroupSlot &g = slots[blockIdx.x / bx];
    if (g.part < 0 || !g.row_ids_map) return;
    int64_t *ids = list_ids + (int64_t)g.part * per_part;
    for (int64_t i = (blockIdx.x % bx) * 256ll + threadIdx.x; i < per_part; i += (int64_t)bx * 256) {
        const int64_t v = ids[i];
        if (v >= 0) ids[i] = (int64_t)g.row_ids_map[v];
    }
}

void launch_bivf_group_map(const BivfGroupSlot *slots, int nentries, int64_t per_part, int64_t *list_ids,
                           hipStream_t s) {
    if (nentries <= 0 || per_part <= 0) return;
    const int bx = (int)std::min<int64_t>((per_part + 255) / 256, 64);
    hipLaunchKernelGGL(k_bivf_group_map, dim3((unsigned)nentries * bx), dim3(256), 0, s, slots, bx, per_part,
                       list_ids);
}

// k_bivf_stats' four sums over every slot of the call (workgroup = table
// entry; stats[4] zeroed by the caller): records kept, non-empty work items,
// list-plane bytes of the probed lists, (query, list) pairs
__global__ __launch_bounds__(256) void k_bivf_group_stats(const BivfGroupSlot *slots, int nq, int code_words,
                                                          const int64_t *probes, const int *count,
                                                          unsigned long long *stats) {
    __shared__ unsigned long long acc[3];
    const BivfGroupSlot &g = slots[blockIdx.x];
    if (g.part < 0) return;  // (a sentinel; block-uniform)
    if (threadIdx.x < 3) acc[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long vals = 0, items = 0, pos = 0;
    for (int i = threadIdx.x; i < nq; i += 256) vals += (unsigned long long)count[g.count0 + i];
    const int64_t E = (int64_t)nq * g.nprobe;
    for (int64_t e = threadIdx.x; e < E; e += 256) {
        const int64_t list = probes[g.probe0 + e];
        if (list < 0 || list >= g.nlist) continue;
        const int64_t len = g.list_off[list + 1] - g.list_off[list];
        pos += (unsigned long long)len;
        items += (unsigned long long)((len + 255) / 256);
    }
    atomicAdd(&acc[0], vals);
    atomicAdd(&acc[1], items);
    atomicAdd(&acc[2], pos);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&stats[0], acc[0]);
        atomicAdd(&stats[1], acc[1]);
        atomicAdd(&stats[2], acc[2] * (unsigned long long)code_words * 4ull);
        atomicAdd(&stats[3], (unsigned long long)E);
    }
}

void launch_bivf_group_stats(const BivfGroupSlot *slots, int nentries, int nq, int code_words, const int64_t *probes,
                             const int *count, int64_t *stats, hipStream_t s) {
    if (nentries <= 0 || nq <= 0) return;
    hipLaunchKernelGGL(k_bivf_group_stats, dim3((unsigned)nentries), dim3(256), 0, s, slots, nq, code_words, probes,
                       count, reinterpret_cast<unsigned long long *>(stats));
}

}  // namespace mqvs
